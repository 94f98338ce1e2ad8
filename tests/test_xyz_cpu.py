"""CPU: quber_amd.camera - the numpy contract of the depth -> point cloud kernel (csrc/dsn.hip xyz_from_depth_kernel).

"uois": xyz_np equals tests/golden/xyz_uois_*.npz, recorded from the reference's own compute_xyz by tools/gen_xyz_golden.py, bit for bit (the
fixtures of the simulated form are float64 where numpy >= 2 recorded them: that tool's docstring says why their float32 rounding is the
float32 evaluation).  "pinhole" has no callable in the reference (eval/base_model.py:489-495 is inline): it is pinned by the formula evaluated
step by step in np.float64 from the integer grid, and shown to differ from the float32 evaluation."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from quber_amd.camera import Camera, check_depth_z, xyz_np

F32_MAX = float(np.finfo(np.float32).max)


def same_bits(got, ref):
    """float32 arrays equal bit for bit, NaN where NaN (whatever its payload)"""
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape
    nan = np.isnan(ref)
    return np.array_equal(nan, np.isnan(got)) and np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))


def fixture_params(f):
    return dict(zip(f["param_keys"].tolist(), f["param_values"].tolist()))


def special_depth(h, w, seed=0):
    """depth with 0, NaN, a negative value, a value near the float32 maximum, inf and a denormal among ordinary metres"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.3, 2.5, (h, w)).astype(np.float32)
    flat = z.reshape(-1)
    special = np.array([F32_MAX * 0.97, 0.0, np.nan, -0.75, np.inf, 1e-42], np.float32)
    pos = rng.choice(flat.size, size=min(len(special), flat.size), replace=False)
    flat[pos] = special[:len(pos)]
    return z


@pytest.mark.parametrize("path", golden("xyz_uois"), ids=os.path.basename)
def test_uois_equals_the_references_compute_xyz(path):
    f = np.load(path)
    z, ref = f["z"], f["xyz"]
    h, w = z.shape
    params = fixture_params(f)
    assert ("fx" in params) == ("explicit" in path) and ("fov" in params) == ("sim" in path)
    if "explicit" in path:
        assert params["x_offset"] != int(params["x_offset"]) and params["y_offset"] != int(params["y_offset"])
    if h * w > 1:
        flat = z.reshape(-1)
        assert (flat == 0).any() and np.isnan(flat).any() and (flat < 0).any()
    assert (z > F32_MAX / 2).any()
    cam = Camera.from_params(params)
    assert cam.convention == "uois"
    got = xyz_np(z, cam)
    assert got.shape == (h, w, 3)
    assert same_bits(got, ref.astype(np.float32))
    assert same_bits(got[..., 2], z)                                    # z passes through untouched
    # a batch is the frames one by one
    zb = np.stack([z, z[::-1].copy()])
    gb = xyz_np(zb, cam)
    assert same_bits(gb[0], got) and same_bits(gb[1], xyz_np(zb[1], cam))


def test_fixture_sizes():
    sizes = sorted({tuple(np.load(p)["z"].shape) for p in golden("xyz_uois")})
    assert sizes == [(1, 1), (3, 5), (48, 80)]
    assert len(golden("xyz_uois")) == 6 and all(os.path.getsize(p) < 128 * 1024 for p in golden("xyz_uois"))


def test_from_params_is_the_references_arithmetic():
    cam = Camera.from_params({"fx": 61.5, "fy": 60.25, "x_offset": 3.3, "y_offset": 2.2, "img_width": 5, "img_height": 3})
    assert cam.params == (61.5, 60.25, 3.3, 2.2) and all(type(v) is float for v in cam.params)
    p = {"fov": 60, "near": 0.01, "img_width": 640, "img_height": 480}
    aspect_ratio = p["img_width"] / p["img_height"]
    e = 1 / (np.tan(np.radians(p["fov"] / 2.)))
    t = p["near"] / e
    r = t * aspect_ratio
    alpha = p["img_width"] / (r - (-r))
    focal = p["near"] * alpha
    cam = Camera.from_params(p)
    assert cam.params == (float(focal), float(focal), 320.0, 240.0) and all(type(v) is float for v in cam.params)
    assert abs(cam.fx - 240.0 / np.tan(np.radians(30.0))) < 1e-12 * cam.fx                  # (h / 2) / tan(fov / 2): the fov is the vertical one


def pinhole_float64(z, fx, fy, cx, cy):
    """eval/base_model.py:489-495 step by step: int64 grid, float64 scalars, float32 depth; one rounding to float32 at the end"""
    h, w = z.shape
    xmap, ymap = np.meshgrid(np.arange(w), np.arange(h))
    assert xmap.dtype == np.int64
    dx = xmap.astype(np.float64) - np.float64(cx)
    qx = dx / np.float64(fx)
    x = qx * z.astype(np.float64)
    dy = ymap.astype(np.float64) - np.float64(cy)
    qy = dy / np.float64(fy)
    y = qy * z.astype(np.float64)
    assert x.dtype == np.float64 and y.dtype == np.float64
    return np.stack([x.astype(np.float32), y.astype(np.float32), z], -1)


def pinhole_float32(z, fx, fy, cx, cy):
    h, w = z.shape
    row, col = np.indices((h, w), dtype=np.float32)
    x = ((col - np.float32(cx)) / np.float32(fx)) * z
    y = ((row - np.float32(cy)) / np.float32(fy)) * z
    assert x.dtype == np.float32
    return np.stack([x, y, z], -1)


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (48, 80)])
def test_pinhole_is_the_float64_formula(shape):
    cam = Camera(1105.0, 1105.0, 511.5, 384.0).scaled(1032, 772, 640, 480)
    assert cam.convention == "pinhole"
    z = special_depth(*shape, seed=3)
    with np.errstate(all="ignore"):
        want = pinhole_float64(z, *cam.params)
    got = xyz_np(z, cam)
    assert same_bits(got, want)
    assert same_bits(got[..., 2], z)
    # rows count from the top: the first row has the smallest y factor
    one = xyz_np(np.ones(shape, np.float32), cam)
    assert (np.diff(one[..., 1], axis=0) > 0).all() and (np.diff(one[..., 0], axis=1) > 0).all()


def test_pinhole_differs_from_the_float32_evaluation():
    """the float64 path is really exercised: on the fixture's depth some pixel rounds differently in float32"""
    z = np.load([p for p in golden("xyz_uois") if "explicit_48x80" in p][0])["z"]
    cam = Camera(1105.0, 1105.0, 511.5, 384.0).scaled(1032, 772, 640, 480)
    with np.errstate(all="ignore"):
        f32 = pinhole_float32(z, *cam.params)
    got = xyz_np(z, cam)
    ok = np.isfinite(got) & np.isfinite(f32)
    differ = ok & (got != f32)
    assert differ[..., :2].any() and not differ[..., 2].any()
    assert np.abs(got[ok] - f32[ok]).max() <= 4 * np.spacing(np.abs(got[ok]).max())          # ... by roundings, not by a different formula


def test_the_two_conventions_differ_in_rows_and_rounding():
    z = special_depth(3, 5, seed=1)
    a, b = xyz_np(z, Camera(61.7, 59.3, 2.13, 1.71, "pinhole")), xyz_np(z, Camera(61.7, 59.3, 2.13, 1.71, "uois"))
    assert same_bits(a[..., 2], b[..., 2]) and not same_bits(a[..., 1], b[..., 1])


def test_scaled_is_the_four_python_expressions():
    cx, cy, fx, fy = 511.5, 384.0, 1105.0, 1105.0
    ori_width, ori_height = 1032, 772
    cx = cx / ori_width * 640
    cy = cy / ori_height * 480
    fx = fx / ori_width * 640
    fy = fy / ori_height * 480
    cam = Camera(1105, 1105, 511.5, 384).scaled(1032, 772, 640, 480)
    assert cam.params == (fx, fy, cx, cy)
    assert Camera(1, 2, 3, 4, "uois").scaled(10, 10, 5, 5).convention == "uois"


def test_camera_and_depth_checks():
    for bad in (lambda: Camera(0.0, 1.0, 0.0, 0.0), lambda: Camera(1.0, float("nan"), 0.0, 0.0), lambda: Camera(1.0, 1.0, float("inf"), 0.0),
                lambda: Camera(1.0, 1.0, 0.0, 0.0, "opengl"), lambda: xyz_np(np.zeros((3, 5), np.float64), Camera(1, 1, 0, 0)),
                lambda: xyz_np(np.zeros(5, np.float32), Camera(1, 1, 0, 0)), lambda: check_depth_z(np.zeros((3, 5), np.float64), 3, 5),
                lambda: check_depth_z(np.zeros((3, 6), np.float32), 3, 5), lambda: check_depth_z(np.zeros((3, 5), np.uint16), 3, 5)):
        with pytest.raises(ValueError):
            bad()
    assert Camera(1, 2, 3, 4) == Camera(1.0, 2.0, 3.0, 4.0) and Camera(1, 2, 3, 4) != Camera(1, 2, 3, 4, "uois")
    assert Camera(1, 2, 3, 4).convention_id == 0 and Camera(1, 2, 3, 4, "uois").convention_id == 1
    z = np.zeros((6, 5), np.float32)[::2]
    assert check_depth_z(z, 3, 5).flags["C_CONTIGUOUS"]


def test_header_and_bindings_declare_the_entries():
    from quber_amd import _lib
    header = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    for name in ("quber_dsn_forward_depth", "quber_dsn_forward_depth_profiled", "quber_op_xyz_from_depth"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in open(os.path.join(ROOT, "quber_amd", "_lib.py")).read(), name
    # the existing entries stay as they are
    assert re.search(r"int quber_dsn_forward\(quber_ctx\* ctx, const float\* dev_xyz, int32_t batch, int32_t flags,", header)
    assert re.search(r"int quber_op_dsn_pack\(const float\* dev_xyz, int32_t batch, int32_t h, int32_t w, int32_t flags, float\* dev_x8, float\* dev_clean, void\* stream\);", header)
    assert _lib is not None


def test_region_and_adapter_options():
    """the options of this feature that need no device: RegionRefinement(final_close_morphology=, ksize=) and the adapters' refusals"""
    from quber_amd import rrn_arch
    from quber_amd.gms import IMP
    from quber_amd.region import RegionRefinement
    sd = rrn_arch.init_state_dict(0, gain=0.7, feature_dim=8)
    off = RegionRefinement(sd)
    assert off.final_close_morphology is False and off.close_imp is None
    on = RegionRefinement(sd, final_close_morphology=True)
    assert on.final_close_morphology is True and on.close_imp == IMP(9, largest=False)
    assert RegionRefinement(sd, final_close_morphology=True, ksize=5).close_imp == IMP(5, largest=False)
    for bad in (lambda: RegionRefinement(sd, final_close_morphology=1), lambda: RegionRefinement(sd, final_close_morphology=True, ksize=4),
                lambda: RegionRefinement(sd, final_close_morphology=True, ksize=17)):
        with pytest.raises(ValueError):
            bad()
    from quber_amd.eval import base_model
    assert base_model.PCD_RULES == {"OSD": "disparity", "OCID": "depth", "HOPE": "depth", "DoPose": "depth"}
    with pytest.raises(FileNotFoundError):
        base_model.pcd_path_for("/nowhere/depth/a.png", "OCID")
    with pytest.raises(ValueError):
        base_model.pcd_path_for("/nowhere/depth/a.png", "WISDOM")
