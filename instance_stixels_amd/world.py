"""The 3-D view of one frame's stixel world, from the records of `host.Stixels.WorldBatch`.

`pointcloud` builds what the reference tooling's `pointcloud()` returns
(tools/visualization/clustering_visualization.py: the object stixels as image points and 3-D points, the ground
stixels as 3-D patches, their classes and the instance ids that feed the top-down view) from a numpy array of
`WORLD_DTYPE` records instead of a parsed `.stixels` file: vectorised, in float64, with the operand order of the
reference's `compute3d`, so that every array has the reference's bits.
"""
import numpy as np

from .config import GROUND, OBJECT
from .core import CONTOUR_DTYPE, OBJECT_DTYPE, WORLD_DTYPE  # noqa: F401  (the dtypes of the record arrays)

FIRST_INSTANCE_CLASS = 11  # IS_FIRST_INSTANCE_CLASS: an object stixel of class >= 11 is an instance candidate


def compute3d(points, camera_parameters):
    """[n][3] (x, y, disparity) in image coordinates (y down) -> [n][3] metres: z = fx * baseline / disparity,
    x = -(z / fx) * (u0 - x), y = -(z / fy) * (v0 - y).  camera_parameters: {'intrinsic': {fx, fy, u0, v0},
    'extrinsic': {baseline}}.  Raises ValueError on a zero disparity."""
    if camera_parameters is None:
        raise ValueError("Camera parameters can not be None anymore!")
    points = np.asarray(points, np.float64).reshape(-1, 3)
    if np.any(points[:, 2] == 0):
        raise ValueError("Divide by zero. Disparity should not be 0.")
    intrinsic = camera_parameters["intrinsic"]
    out = np.empty(points.shape)
    out[:, 2] = (intrinsic["fx"] * camera_parameters["extrinsic"]["baseline"]) / points[:, 2]
    out[:, 0] = -(out[:, 2] / intrinsic["fx"]) * (intrinsic["u0"] - points[:, 0])
    out[:, 1] = -(out[:, 2] / intrinsic["fy"]) * (intrinsic["v0"] - points[:, 1])
    return out


def instance_ids(records):
    """Per record the Cityscapes-style instance id the reference's reader makes of a cluster label:
    semantic_class * 1000 + label for 0 <= label < 1000, else -1."""
    label = records["instance_id"].astype(np.int64)
    return np.where((label >= 0) & (label < 1000), records["semantic_class"].astype(np.int64) * 1000 + label, -1)


def pointcloud(records, image_shape, groundplane, camera_parameters, realcols):
    """records: the WORLD_DTYPE records of ONE frame, in (column, section) order; image_shape: (rows, cols);
    groundplane: (alpha_ground, vhor) with vhor in the library's convention (StixelsData.vhor, what SaveStixels
    writes); realcols: the stixel columns of the frame (Stixels.GetRealCols(); the reference takes it from the
    length of its per-column list, and the records cannot tell it: a trailing column may hold no stixel).  Returns
    the reference's dictionary:
      points [n_obj][3] (mean x, mean y, disparity), points3d [n_obj][3], pixels [n_obj] rows per object stixel,
      object_semantics [n_obj], ground_patches3d [n_gnd][4][3] (TL, TR, BR, BL), ground_semantics [n_gnd],
      instances: per object stixel that is an instance candidate (class >= 11) its instance id, -1 = none.
    Raises ValueError where the reference does: a zero disparity among the object points or patch corners."""
    records = np.asarray(records)
    rows, cols = int(image_shape[0]), int(image_shape[1])
    if int(realcols) < 1 or (records.size and int(records["column"].max()) >= int(realcols)):
        raise ValueError("pointcloud: realcols does not hold the records' columns")
    width = cols // int(realcols)
    left = records["column"].astype(np.int64) * width
    top = rows - records["vT"].astype(np.int64) - 1
    right = left + width - 1
    bottom = rows - records["vB"].astype(np.int64) - 1

    obj = records["type"] == OBJECT
    gnd = records["type"] == GROUND
    points = np.empty((int(obj.sum()), 3))
    points[:, 0] = 0.5 * (left[obj] + right[obj] + 1)
    points[:, 1] = 0.5 * (top[obj] + bottom[obj])
    points[:, 2] = records["disparity"][obj]
    pixels = bottom[obj] - top[obj] + 1
    candidate = records["semantic_class"][obj] >= FIRST_INSTANCE_CLASS

    alpha, vhor = float(groundplane[0]), int(groundplane[1])
    top_disparity = alpha * (vhor - records["vT"][gnd].astype(np.int64)).astype(np.float64)
    bottom_disparity = alpha * (vhor - records["vB"][gnd].astype(np.int64)).astype(np.float64)
    patches = np.empty((int(gnd.sum()), 4, 3))
    patches[:, 0, 0] = patches[:, 3, 0] = left[gnd]
    patches[:, 1, 0] = patches[:, 2, 0] = right[gnd]
    patches[:, 0, 1] = patches[:, 1, 1] = top[gnd]
    patches[:, 2, 1] = patches[:, 3, 1] = bottom[gnd]
    patches[:, 0, 2] = patches[:, 1, 2] = top_disparity
    patches[:, 2, 2] = patches[:, 3, 2] = bottom_disparity

    points3d = compute3d(points, camera_parameters)
    patches3d = compute3d(patches.reshape(-1, 3), camera_parameters).reshape(patches.shape)
    return {"points3d": points3d, "points": points, "pixels": pixels, "ground_patches3d": patches3d,
            "ground_semantics": records["semantic_class"][gnd].astype(np.int64),
            "object_semantics": records["semantic_class"][obj].astype(np.int64),
            "instances": instance_ids(records[obj])[candidate]}


def instance_objects(objects, points, image_shape, realcols, camera_parameters):
    """The per-instance view of a batch from the two arrays of `host.Stixels.InstanceObjectsBatch`: objects
    (OBJECT_DTYPE) and points (CONTOUR_DTYPE); image_shape: (rows, cols); realcols: the stixel columns of a frame.
    Returns a dictionary, one entry per object in the arrays' order:
      mean_disparity [n] float64: the pixel-weighted mean disparity, disparity_q16_sum / (65536 * pixels / w) with
                     w = cols // realcols (NaN for an object without pixels);
      box [n][4] int64: (left, top, right, bottom) in image pixels, inclusive -- col_min * w, top, col_max * w + w - 1,
                     bottom; an object without pixels has top = rows and bottom = -1;
      contour_offsets [n + 1]: object o owns contour[contour_offsets[o]:contour_offsets[o + 1]] (its first_point and
                     n_columns), ascending by stixel column;
      contour [m][3] float64: per contour point the image point the reference's pointcloud() gives that stixel
                     (mean x, mean y, disparity); contour3d [m][3]: the same through compute3d, in metres;
      closest_distance [n] float64: the smallest Euclidean distance sqrt(x^2 + y^2 + z^2) of the object's contour
                     points, the measure the reference's top-down view ranks stixels by.
    A contour point is the DEPTH-closest stixel of the object in its column (the largest disparity).  The reference's
    plot instead takes the Euclidean-closest stixel of the column after dropping stixels more than 3 m off the
    instance's median depth; a caller that wants that choice applies it to the per-stixel records of WorldBatch --
    the few contour points here are the cheap form.  Raises ValueError where compute3d raises: a zero disparity
    among the contour points, or camera_parameters None."""
    objects, points = np.asarray(objects), np.asarray(points)
    rows, cols = int(image_shape[0]), int(image_shape[1])
    if int(realcols) < 1 or (objects.size and int(objects["col_max"].max()) >= int(realcols)):
        raise ValueError("instance_objects: realcols does not hold the objects' columns")
    first = objects["first_point"].astype(np.int64)
    count = objects["n_columns"].astype(np.int64)
    if objects.size and (first[0] != 0 or np.any(first[1:] != first[:-1] + count[:-1])
                         or first[-1] + count[-1] != len(points)):
        raise ValueError("instance_objects: the points are not those of the objects")
    width = cols // int(realcols)
    pixels = objects["pixels"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_disparity = np.where(pixels > 0, objects["disparity_q16_sum"].astype(np.float64)
                                  / (65536.0 * pixels / width), np.nan)
    box = np.stack([objects["col_min"].astype(np.int64) * width, objects["top"].astype(np.int64),
                    objects["col_max"].astype(np.int64) * width + width - 1, objects["bottom"].astype(np.int64)],
                   axis=1).reshape(-1, 4)
    left = points["column"].astype(np.int64) * width
    right = left + width - 1
    top = rows - points["vT"].astype(np.int64) - 1
    bottom = rows - points["vB"].astype(np.int64) - 1
    contour = np.empty((len(points), 3))
    contour[:, 0] = 0.5 * (left + right + 1)
    contour[:, 1] = 0.5 * (top + bottom)
    contour[:, 2] = points["disparity"]
    contour3d = compute3d(contour, camera_parameters)
    distance = np.sqrt((contour3d ** 2).sum(axis=1))
    offsets = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    closest = np.array([distance[offsets[o]:offsets[o + 1]].min() for o in range(len(objects))], np.float64)
    return {"mean_disparity": mean_disparity, "box": box, "contour_offsets": offsets, "contour": contour,
            "contour3d": contour3d, "closest_distance": closest}
