#!/usr/bin/env python
"""Record tests/golden/losstargets_*.npz from the reference's own PanopticDeepLabTargetGenerator
(maskrefiner/data/dataset_mappers/target_generator.py:8-165).  Run by hand where a checkout of the reference is at hand:

    python tools/gen_loss_golden.py --reference /path/to/QuBER

The module is loaded by path with a stand-in for cv2, which only its PerturbedInputGenerator uses.  Every segment is a thing and none is
crowd, as in the datasets the reference trains on.  The fixtures hold arrays only: the label map, the parameters and what the generator
returned.  The numpy of the recording process decides the offset arithmetic (`float64 scalar - float32 array`): numpy >= 2 records
mode 0 (quber_config.encode_legacy_f32 = 0), which is what the fixtures pin."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator(reference):
    path = os.path.join(reference, "maskrefiner", "data", "dataset_mappers", "target_generator.py")
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("reference_target_generator", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PanopticDeepLabTargetGenerator


def box(lab, y0, y1, x0, x1, i):
    lab[y0:y1, x0:x1] = i


def cases():
    """name -> (labels i32 [H,W], n, sigma, small_area, small_weight)"""
    out = {}
    lab = np.zeros((37, 53), np.int32)                               # sigma 10: the 63-pixel window is clipped on all four sides
    box(lab, 14, 23, 20, 33, 1)
    box(lab, 2, 8, 3, 12, 2)
    box(lab, 30, 37, 44, 53, 3)
    out["clip_37x53_s10"] = (lab, 3, 10, 60, 3)
    rng = np.random.default_rng(77)
    lab = np.zeros((96, 128), np.int32)
    yy, xx = np.mgrid[:96, :128]
    for i in range(1, 9):
        cy, cx, ry, rx = rng.integers(0, 96), rng.integers(0, 128), rng.integers(3, 30), rng.integers(3, 40)
        lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = i
    out["scene_96x128_s8"] = (lab, 8, 8, 700, 3)
    lab = np.zeros((24, 40), np.int32)
    box(lab, 1, 4, 1, 6, 1)
    box(lab, 10, 20, 18, 25, 2)
    box(lab, 22, 24, 38, 40, 3)
    out["sigma1_24x40_s1"] = (lab, 3, 1, 10, 2)
    lab = np.zeros((20, 24), np.int32)                               # two-pixel instances whose centre is x.5: ties to even
    lab[3, 4:6] = 1                                                  # cx 4.5 -> 4
    lab[3, 11:13] = 2                                                # cx 11.5 -> 12
    lab[8:10, 7] = 3                                                 # cy 8.5 -> 8
    lab[13:15, 20] = 4                                               # cy 13.5 -> 14
    lab[17:19, 0] = 5                                                # cy 17.5 -> 18, at the left edge
    out["ties_20x24_s2"] = (lab, 5, 2, 0, 1)
    lab = np.zeros((64, 96), np.int32)                               # areas small_area - 1 and small_area
    box(lab, 4, 9, 4, 10, 1)                                         # 30
    lab[8, 9] = 0                                                    # 29
    box(lab, 20, 25, 50, 56, 2)                                      # 30
    box(lab, 40, 60, 10, 40, 3)                                      # 600
    out["small_64x96_s4"] = (lab, 3, 4, 30, 3)
    lab = np.zeros((32, 48), np.int32)                               # a declared id with no pixel
    box(lab, 2, 12, 2, 20, 1)
    box(lab, 16, 30, 24, 46, 3)
    box(lab, 20, 24, 30, 36, 4)
    out["absent_32x48_s3"] = (lab, 4, 3, 40, 5)
    out["empty_16x16_s2"] = (np.zeros((16, 16), np.int32), 0, 2, 10, 3)
    lab = np.zeros((40, 60), np.int32)                               # overlapping windows: the maximum decides
    box(lab, 15, 22, 20, 27, 1)
    box(lab, 17, 24, 29, 36, 2)
    out["overlap_40x60_s5"] = (lab, 2, 5, 10, 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    gen_cls = load_generator(args.reference)
    for name, (lab, n, sigma, small_area, small_weight) in cases().items():
        gen = gen_cls(ignore_label=255, thing_ids=[1], sigma=sigma, ignore_stuff_in_offset=True, small_instance_area=small_area,
                      small_instance_weight=small_weight, ignore_crowd_in_semantic=False)
        r = gen(lab, [{"id": i, "category_id": 1, "iscrowd": 0} for i in range(1, n + 1)])
        path = os.path.join(args.out, "losstargets_%s.npz" % name)
        np.savez_compressed(
            path, labels=lab.astype(np.uint8), params=np.array([sigma, n, small_area, small_weight], np.int32),
            numpy_version=np.array(np.__version__), center=r["center"].numpy().astype(np.float32), offset=r["offset"].numpy().astype(np.float32),
            sem_seg=r["sem_seg"].numpy().astype(np.uint8), sem_seg_weights=r["sem_seg_weights"].numpy().astype(np.float32),
            center_weights=r["center_weights"].numpy()[0].astype(np.uint8), offset_weights=r["offset_weights"].numpy()[0].astype(np.uint8),
            center_points=np.asarray(r["center_points"], np.float64).reshape(-1, 2),
            area=np.bincount(lab.ravel(), minlength=n + 1)[1:n + 1].astype(np.int32))
        print("%-28s %6d bytes" % (os.path.basename(path), os.path.getsize(path)))


if __name__ == "__main__":
    main()
