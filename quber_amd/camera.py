"""A camera's four intrinsics and the two ways the reference turns a depth image into an organised point cloud.

``xyz_np(z, cam)`` states both in numpy; it is the contract the device kernel (csrc/dsn.hip xyz_from_depth_kernel) is held to, bit for bit.

  * ``"pinhole"`` (reference eval/base_model.py:489-495, the intrinsics branch of ``UOISNet.predict``): float64 arithmetic from the
    integer pixel grid, ``x = ((col - cx) / fx) * z``, ``y = ((row - cy) / fy) * z``, every operation rounded on its own, the result
    rounded to float32 once (array_to_tensor's ``.float()``).  Rows count from the top; the y negation of :498 is bit 0 of the Depth
    Seeding Network's flags, not part of this function.
  * ``"uois"`` (reference eval/preprocess_utils.py:96-139 ``compute_xyz``): float32 arithmetic, because build_matrix_of_indices is
    float32 and a Python scalar does not widen it: ``x = ((col - x_offset) * z) / fx``, ``y = (((H - 1 - row) - y_offset) * z) / fy``
    with the four scalars rounded to float32 first.  The row index is flipped (``np.flipud``).

NaN, inf, 0 and negative depths pass through the arithmetic unchanged; NaN -> 0 is the Depth Seeding Network's own rule, applied after."""
import math

import numpy as np

CONVENTIONS = ("pinhole", "uois")


class Camera:
    """fx, fy, cx, cy as Python floats (cx, cy are compute_xyz's x_offset, y_offset) and the convention of the back-projection."""

    def __init__(self, fx, fy, cx, cy, convention="pinhole"):
        if convention not in CONVENTIONS:
            raise ValueError(f"Camera: convention {convention!r}, expected one of {CONVENTIONS}")
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        if not all(math.isfinite(v) for v in self.params) or self.fx == 0.0 or self.fy == 0.0:
            raise ValueError(f"Camera: fx, fy, cx, cy must be finite and the focal lengths other than zero (got {self.params})")
        self.convention = convention

    @property
    def params(self):
        return (self.fx, self.fy, self.cx, self.cy)

    @property
    def convention_id(self):
        return CONVENTIONS.index(self.convention)

    def __repr__(self):
        return "Camera(fx=%r, fy=%r, cx=%r, cy=%r, convention=%r)" % (self.params + (self.convention,))

    def __eq__(self, other):
        return isinstance(other, Camera) and self.params == other.params and self.convention == other.convention

    __hash__ = None

    @classmethod
    def from_params(cls, camera_params, convention="uois"):
        """compute_xyz's reading of a camera_params dict: fx / fy and x_offset / y_offset where present, otherwise (simulated data) the
        focal length from fov (degrees), near, img_width and img_height, and the image centre as the offsets.  Python floats in the
        reference's order of operations."""
        p = camera_params
        if "fx" in p and "fy" in p:
            fx, fy = float(p["fx"]), float(p["fy"])
        else:
            aspect_ratio = p["img_width"] / p["img_height"]
            e = 1 / float(np.tan(np.radians(p["fov"] / 2.)))      # numpy's tan, as the reference calls it; Python floats from here on
            t = p["near"] / e
            r = t * aspect_ratio
            alpha = p["img_width"] / (r - (-r))           # pixels per metre
            fx = fy = p["near"] * alpha
        if "x_offset" in p and "y_offset" in p:
            cx, cy = float(p["x_offset"]), float(p["y_offset"])
        else:
            cx, cy = p["img_width"] / 2, p["img_height"] / 2
        return cls(fx, fy, cx, cy, convention)

    def scaled(self, ori_w, ori_h, w, h):
        """the intrinsics of the frame resized from ori_w x ori_h to w x h (eval/base_model.py:485-488: divide, then multiply)"""
        return Camera(self.fx / ori_w * w, self.fy / ori_h * h, self.cx / ori_w * w, self.cy / ori_h * h, self.convention)


def xyz_np(z, cam):
    """z f32 [H,W] or [B,H,W] in metres -> f32 [...,H,W,3], the organised point cloud of ``cam`` in its convention."""
    z = np.asarray(z)
    if z.dtype != np.float32 or z.ndim not in (2, 3):
        raise ValueError(f"xyz_np: depth must be float32 [H,W] or [B,H,W], got {z.dtype} {z.shape}")
    H, W = z.shape[-2:]
    with np.errstate(all="ignore"):
        if cam.convention == "pinhole":
            col, row = np.meshgrid(np.arange(W), np.arange(H))
            fx, fy, cx, cy = (np.float64(v) for v in cam.params)
            zd = z.astype(np.float64)
            x = (((col - cx) / fx) * zd).astype(np.float32)
            y = (((row - cy) / fy) * zd).astype(np.float32)
        else:
            row, col = np.indices((H, W), dtype=np.float32)
            row = np.flipud(row)
            fx, fy, cx, cy = (np.float32(v) for v in cam.params)
            x = ((col - cx) * z) / fx
            y = ((row - cy) * z) / fy
            assert x.dtype == np.float32 and y.dtype == np.float32
        x, y = np.broadcast_to(x, z.shape), np.broadcast_to(y, z.shape)
    return np.stack([x, y, z], axis=-1)


def check_depth_z(z, h, w, who="depth_z"):
    """one depth plane of a camera= call -> contiguous float32 [h,w] host array; ValueError for another shape or dtype"""
    if hasattr(z, "detach"):
        z = z.detach().cpu().numpy()
    z = np.asarray(z)
    if z.dtype != np.float32 or z.shape != (h, w):
        raise ValueError(f"{who}: expected float32 [{h},{w}] in metres, got {z.dtype} {z.shape}")
    return np.ascontiguousarray(z)
