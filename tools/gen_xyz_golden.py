#!/usr/bin/env python3
"""Records tests/golden/xyz_uois_*.npz: depth images and camera parameters run through the reference's own ``compute_xyz``
(eval/preprocess_utils.py:96-139), imported unmodified by file path with an empty stand-in for ``cv2`` in sys.modules (compute_xyz does not
use it; the module imports it).  TEST INFRASTRUCTURE for the machine that holds the reference: nothing of it is copied here beyond the
inputs and the recorded outputs.  tests/test_xyz_cpu.py holds quber_amd.camera.xyz_np ("uois") to these files, bit for bit.

usage: python3 tools/gen_xyz_golden.py [--reference DIR]   -> tests/golden/xyz_uois_<form>_<h>x<w>.npz

Cases: the explicit fx / fy / x_offset / y_offset form with non-integer offsets, and the simulated fov / near form, at 1 x 1, 3 x 5 and
48 x 80; every depth image holds 0, NaN, a negative value and a value near the float32 maximum.

The simulated form and numpy >= 2: there the reference's focal length is an np.float64 scalar (it comes out of np.tan), which widens the
one division by it to float64 (a Python float, the explicit form, does not), and compute_xyz returns float64.  Under numpy 1 the whole
expression stays float32, which is the contract.  The simulated cases use fov 90 / near 0.01, for which the focal length is w / 2 up to one
part in 2^52: a float32 number at 3 x 5 and 48 x 80 (dividing two float32 numbers in float64 and rounding once more gives the float32
quotient), and at 1 x 1 0.5 (1 + 2^-52), where the quotient is a float32 number scaled by (1 - 2^-52) and rounds back to it.  So the
recorded values, rounded to float32, are those of either numpy generation; the file records the dtype it got and numpy's version."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
F32_MAX = float(np.finfo(np.float32).max)


def reference_compute_xyz(ref):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_preprocess_utils", os.path.join(ref, "eval", "preprocess_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.compute_xyz


def depth_image(h, w, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.3, 2.5, (h, w)).astype(np.float32)
    flat = z.reshape(-1)
    special = np.array([0.0, np.nan, -0.75, F32_MAX * 0.97, np.inf, 1e-42], np.float32)   # (1 x 1: the value near the float32 maximum alone)
    if flat.size == 1:
        flat[0] = special[3]
    else:
        pos = rng.choice(flat.size, size=min(len(special), flat.size), replace=False)
        flat[pos] = special[:len(pos)]
    return z


def cases():
    for i, (h, w) in enumerate(((1, 1), (3, 5), (48, 80))):
        yield "explicit", h, w, {"fx": 61.7 + 0.13 * w, "fy": 59.3 + 0.11 * h, "x_offset": w / 2 - 0.37, "y_offset": h / 2 + 0.21,
                                 "img_width": w, "img_height": h}, 10 + i
        yield "sim", h, w, {"fov": 90, "near": 0.01, "img_width": w, "img_height": h}, 20 + i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    compute_xyz = reference_compute_xyz(args.reference)
    os.makedirs(OUT, exist_ok=True)
    for form, h, w, params, seed in cases():
        z = depth_image(h, w, seed)
        with np.errstate(all="ignore"):
            xyz = compute_xyz(z.copy(), dict(params))
        assert xyz.shape == (h, w, 3), xyz.shape
        keys = sorted(params)
        path = os.path.join(OUT, "xyz_uois_%s_%dx%d.npz" % (form, h, w))
        np.savez_compressed(path, z=z, xyz=xyz, param_keys=np.array(keys), param_values=np.array([float(params[k]) for k in keys], np.float64),
                            numpy_version=np.array(np.__version__))
        print("%s: %s %s, %d NaN" % (os.path.relpath(path, ROOT), xyz.dtype, xyz.shape, int(np.isnan(xyz).sum())))


if __name__ == "__main__":
    main()
