"""Writes tests/golden/reference_hip/*.npz: small cases recorded from the upstream reference's OWN code
(hipified, built for gfx950 into oracle/_ref/libref_stixels.so by `make -C oracle ref`).

PROVENANCE: the expected outputs come from the reference's Stixels class run on an MI355X through
oracle/ref_driver.hip, under the numerics substitutions of oracle/ref_shim.h.  They let
tests/test_oracle_vs_reference_golden.py hold the oracle to the reference on any machine, without a GPU
and without the reference.  Needs a GPU and the built library.  Run from the repo root:
    python tests/golden/make_reference_golden.py

Each file holds the case (preset, shape, overrides as JSON), the frame's inputs, and the reference's
outputs: Sections, joined disparity, object-LUT rows 0..H, the instance candidates per class as a
sorted multiset, and the vhor it derived.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
from oracle import reference  # noqa: E402

# name: (preset, rows, cols, max_dis, overrides, input variant)
CASES = {
    "unary_64x64x32": ("drn_d_22_unary", 64, 64, 32, {}, None),
    "pairwise_64x64x32": ("drn_d_38_pairwise", 64, 64, 32, {}, None),
    "unary_invalid0_72x64x24": ("drn_d_38_unary", 72, 64, 24, dict(invalid_disparity=0.0), None),
    "pairwise_invalid0_72x64x24": ("drn_d_22_pairwise", 72, 64, 24, dict(invalid_disparity=0.0), None),
    "pairwise_median_invalid0_64x64x32": ("drn_d_38_pairwise", 64, 64, 32,
                                          dict(invalid_disparity=0.0, median_join=True), None),
    "unary_median_64x64x32": ("drn_d_22_unary", 64, 64, 32, dict(median_join=True), None),
    "disparity_only_pairwise_64x64x32": ("disparity_only_pairwise", 64, 64, 32, {}, None),
    "hostile_pairwise_64x64x32": ("drn_d_38_pairwise", 64, 64, 32, {}, "hostile"),
    "hostile_unary_invalid0_64x64x32": ("drn_d_22_unary", 64, 64, 32, dict(invalid_disparity=0.0), "hostile"),
    "degenerate_pairwise_invalid0_64x64x32": ("drn_d_22_pairwise", 64, 64, 32, dict(invalid_disparity=0.0),
                                              "degenerate"),
    "degenerate_unary_invalid0_64x64x32": ("drn_d_38_unary", 64, 64, 32, dict(invalid_disparity=0.0),
                                           "degenerate"),
    "homogeneous_pairwise_64x64x32": ("drn_d_38_pairwise", 64, 64, 32, {}, "homogeneous"),
}
SEED = 41


def degenerate(case):
    """Columns where DP candidates tie: all invalid, constant disparity, zero or all-equal class
    values (the tie rules of the DP and of the class argmin decide these)."""
    d, s = case["disparity"][0], case["segmentation"][0]
    d[:, 0:8] = 0.0            # column 0: every pixel invalid
    d[:, 8:16] = 5.0           # column 1: constant disparity
    d[32:, 16:24] = 0.0        # column 2: lower half invalid
    s[3] = 0                   # column 3: zero segmentation
    s[4, :19] = 0              # column 4: all classes tie, offsets kept
    d[:, 40:48] = 12.0         # column 5: constant disparity and
    s[5] = 0                   #           zero segmentation
    return case


def case_of(preset, rows, cols, D, ov, variant):
    case = helpers.build_case(preset, rows, cols, D, seed=SEED, **ov)
    if variant == "hostile":
        return helpers.make_hostile(case, SEED)
    if variant == "degenerate":
        return degenerate(case)
    if variant is not None:        # an input family of instance_stixels_amd.synthetic
        from instance_stixels_amd import synthetic
        from oracle import oracle
        cfg = case["cfg"]
        f = synthetic.make_frame(cfg, seed=SEED, family=variant)
        g = oracle.host_ground(cfg, f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground)
        case["frames"] = [f]
        case["gf"][0], case["ng"][0], case["ig"][0], case["vhor"][0] = g
        case["disparity"][0], case["segmentation"][0] = f.disparity, f.segmentation
    return case


def candidates(out):
    """All classes' candidate multisets, concatenated, with the class in front."""
    recs = []
    for cls in range(reference.INSTANCE_CLASSES):
        r = reference.candidate_multiset(out, cls)
        recs.append(np.stack([np.full(len(r), cls, np.int64), r["col"], r["i"], r["x"], r["y"], r["core"]], 1))
    return np.concatenate(recs).astype(np.int64).reshape(-1, 6)


if __name__ == "__main__":
    out_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_hip")
    os.makedirs(out_dir, exist_ok=True)
    for name, (preset, rows, cols, D, ov, variant) in CASES.items():
        case = case_of(preset, rows, cols, D, ov, variant)
        f = case["frames"][0]
        ref = reference.stixels_compute_frame(case, want_lut=True)
        C = case["cfg"].realcols
        n = [helpers.n_sections(ref["sections"][c]) for c in range(C)]
        sections = np.zeros((C, max(n) + 1, 8), np.int32)    # up to and including each terminator
        for c in range(C):
            sections[c, : n[c] + 1] = ref["sections"][c][: n[c] + 1].view(np.int32).reshape(-1, 8)
            sections[c, n[c]:, 0] = -1
            sections[c, n[c]:, 1:] = 0                        # (the terminator's other fields are unset)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(
            path, case=json.dumps(dict(preset=preset, rows=rows, cols=cols, max_dis=D, overrides=ov)),
            disparity=case["disparity"][0], segmentation=case["segmentation"][0],
            road=np.array([f.vhor_image, f.camera_tilt, f.camera_height, f.alpha_ground], np.float64),
            sections=sections, joined=ref["joined"], object_lut=ref["object_lut"][:, :, : rows + 1],
            inst_per_class=ref["inst_per_class"], candidates=candidates(ref), vhor=np.int32(ref["vhor"]))
        print(f"{path}: {os.path.getsize(path)} bytes, {sum(n)} sections, "
              f"{int(ref['inst_per_class'].sum())} instance candidates")
