"""numpy restatement of is_cluster_instance_disparity / Stixels::ClusterInstanceDisparityBatch (f10), for the tests --
not a test itself.  Written from the rules of the entry point (instance_stixels_core.h), which restate the reference
tooling's --use-disparity from_gt (compute_instance_disparity, add_instance_disparity, get_disparity_instance_centers
and assign_instances of tools/visualization/clustering_visualization.py over load_instance_mask):

1. a ground-truth pixel id has a key when id > 1000 and id // 1000 is one of 24, 25, 26, 27, 28, 31, 32, 33;
   key = class index * 1000 + id % 1000.  A key's median is np.median of the non-zero disparity_u8 values under it
   (0 where it has none), kept in half units; every other pixel has the instance disparity 0;
2. a section in front of its column's terminator with class 11..18 takes np.median of the instance disparities >= 1
   inside its rectangle (image rows rows-1-vT .. rows-1-vB, columns column*w .. column*w + w-1, clipped; w = cols //
   realcols), 0 where nothing is left; every other slot 0;
3. the candidates of a class are its object sections in (column, section) order; those whose median is 0 take no part
   and get -1; over the others the rules of oracle.cluster_instances hold with dx*dx + dy*dy + dz*dz in float32
   against eps*eps, the core-candidate flag being vT + 1 - vB >= size_filter.
"""
import numpy as np

CITYSCAPES_LABEL_IDS = (24, 25, 26, 27, 28, 31, 32, 33)
KEYS = 8000


def column_count(col):
    t = np.nonzero(col["type"] == -1)[0]
    return int(t[0]) if t.size else len(col)


def pixel_keys(gt):
    """The key of every pixel, -1 where it has none."""
    v = np.asarray(gt, np.int64)
    L = v // 1000
    ci = np.full(v.shape, -1, np.int64)
    for i, lab in enumerate(CITYSCAPES_LABEL_IDS):
        ci[(v > 1000) & (L == lab)] = i
    return np.where(ci >= 0, ci * 1000 + v % 1000, -1).astype(np.int32)


def key_medians(gt, disparity_u8):
    """One frame: (median of every key in half units, uint16 [KEYS]; number of keys present)."""
    keys = pixel_keys(gt).ravel()
    d = np.asarray(disparity_u8, np.uint8).ravel()
    half = np.zeros(KEYS, np.uint16)
    present = np.unique(keys[keys >= 0])
    for k in present.tolist():
        vals = d[keys == k]
        vals = vals[vals != 0]
        if vals.size:
            m = float(np.median(vals.astype(np.float64)))
            assert m * 2 == int(m * 2)
            half[k] = int(m * 2)
    return half, int(present.size)


def stixel_medians(sections, gt, half):
    """One frame: float32 [realcols][max_sections], the median of every instance-class stixel."""
    C, S = sections.shape
    rows, cols = gt.shape
    w = cols // C
    keys = pixel_keys(gt)
    inst = np.where(keys >= 0, half[np.maximum(keys, 0)].astype(np.float64) * 0.5, 0.0)   # the reference's image
    out = np.zeros((C, S), np.float32)
    for c in range(C):
        col = sections[c]
        for i in range(column_count(col)):
            if not 11 <= int(col[i]["semantic_class"]) <= 18:
                continue
            vB, vT = int(col[i]["vB"]), int(col[i]["vT"])
            top, bot = max(rows - 1 - vT, 0), min(rows - 1 - vB, rows - 1)
            if top > bot:
                continue
            px = inst[top:bot + 1, c * w:c * w + w].ravel()
            px = px[px >= 1]
            if px.size:
                m = float(np.median(px))
                assert np.float32(m) == m and m * 4 == int(m * 4)
                out[c, i] = m
    return out


def candidates(sections, cls):
    """(column, section) of the candidates of class 11 + cls in the order of d_indices."""
    out = []
    for c in range(sections.shape[0]):
        col = sections[c]
        for i in range(column_count(col)):
            if int(col[i]["type"]) == 1 and int(col[i]["semantic_class"]) == 11 + cls:
                out.append((c, i))
    return np.array(out, np.int32).reshape(-1, 2)


def cluster3(xyz, large, eps, min_pts):
    """oracle.cluster_instances over three float32 coordinates; every point takes part."""
    X = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    cand = np.asarray(large, bool).reshape(-1)
    n = X.shape[0]
    labels = np.full(n, -1, np.int32)
    big = np.nonzero(cand)[0]
    if n == 0 or big.size <= min_pts:
        return labels
    eps2 = np.float32(eps) * np.float32(eps)

    def d2(a, b):  # [len(a)][len(b)] float32, (dx*dx + dy*dy) + dz*dz, no contraction
        dx = X[a, 0][:, None] - X[b, 0][None, :]
        dy = X[a, 1][:, None] - X[b, 1][None, :]
        dz = X[a, 2][:, None] - X[b, 2][None, :]
        return (dx * dx + dy * dy) + dz * dz

    with np.errstate(invalid="ignore", over="ignore"):
        near = d2(big, big) <= eps2
    is_core = near.sum(axis=1) >= min_pts
    lab = np.full(big.size, -1, np.int32)
    nxt = 0
    for seed in range(big.size):                       # sklearn's dbscan_inner, in index order
        if lab[seed] != -1 or not is_core[seed]:
            continue
        stack = [seed]
        while stack:
            i = stack.pop()
            if lab[i] == -1:
                lab[i] = nxt
                if is_core[i]:
                    stack.extend(int(v) for v in np.nonzero(near[i] & (lab == -1))[0])
        nxt += 1
    labels[big] = lab
    cores = big[is_core]
    small = np.nonzero(~cand)[0]
    if cores.size and small.size:
        with np.errstate(invalid="ignore", over="ignore"):
            dist = d2(small, cores)
        dist = np.where(np.isnan(dist), np.float32(np.inf), dist)
        closest = dist.argmin(axis=1)
        dmin = dist[np.arange(small.size), closest]
        ok = dmin <= eps2
        labels[small[ok]] = labels[cores[closest[ok]]]
    return labels


def cluster_frame(sections, medians, eps, min_pts, size_filter):
    """One frame: per class (indices [n][2], labels [n], core flags [n]) and the per-section label map."""
    C, S = sections.shape
    per_class = []
    label_map = np.full((C, S), -1, np.int32)
    for cls in range(8):
        idx = candidates(sections, cls)
        sec = sections[idx[:, 0], idx[:, 1]]
        z = medians[idx[:, 0], idx[:, 1]]
        large = (sec["vT"].astype(np.int64) + 1 - sec["vB"]) >= size_filter
        labels = np.full(len(idx), -1, np.int32)
        part = np.nonzero(z != 0)[0]
        if part.size:
            xyz = np.stack([sec["instance_meanx"][part], sec["instance_meany"][part], z[part]], 1)
            labels[part] = cluster3(xyz, large[part], eps, min_pts)
        label_map[idx[:, 0], idx[:, 1]] = labels
        per_class.append((idx, labels, large.astype(np.uint8)))
    return per_class, label_map


def run(sections, gt, disparity_u8, eps, min_pts, size_filter):
    """sections [n][realcols][max_sections] SECTION_DTYPE, gt int32 and disparity_u8 uint8 [n][rows][cols] ->
    dict(key_median uint16 [n][KEYS], key_count [n], stixel_median float32 [n][C][S], label_map int32 [n][C][S],
    per_class: per frame the list of cluster_frame, packed: per frame the (column, section, label) triples, classes
    ascending, mappings: per frame {(column, section): label} of every candidate)."""
    n = sections.shape[0]
    out = dict(key_median=[], key_count=[], stixel_median=[], label_map=[], per_class=[], packed=[], mappings=[])
    for f in range(n):
        half, count = key_medians(gt[f], disparity_u8[f])
        med = stixel_medians(sections[f], gt[f], half)
        per_class, label_map = cluster_frame(sections[f], med, eps, min_pts, size_filter)
        tri = np.concatenate([np.concatenate([idx, lab[:, None]], 1) for idx, lab, _ in per_class]).astype(np.int32)
        out["key_median"].append(half)
        out["key_count"].append(count)
        out["stixel_median"].append(med)
        out["label_map"].append(label_map)
        out["per_class"].append(per_class)
        out["packed"].append(tri.reshape(-1, 3))
        out["mappings"].append({(int(c), int(s)): int(l) for c, s, l in tri.reshape(-1, 3).tolist()})
    for k in ("key_median", "key_count", "stixel_median", "label_map"):
        out[k] = np.stack([np.asarray(v) for v in out[k]])
    return out
