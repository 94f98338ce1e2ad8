"""Drop-in for the reference's ``eval/base_model.py:UOISNet`` (reference lines 441-520): ``UOISNet(...).predict(rgb_path, depth_path) ->
(pred_masks bool [K,H,W], fg_mask bool [H,W], seconds)``, UOIS-Net-3D from files to masks with every stage on the device:
Depth Seeding Network -> Gaussian mean shift -> IMP -> crops, Region Refinement Network, paste (-> final close).  No refiner network is
constructed; the stages are those ``MaskRefinerPredictor(seeding=, cluster=, region=)`` runs (quber_amd/uois_chain.py).

The point cloud comes from the ``.pcd`` file beside the depth file, found by the reference's two path rules (``'disparity' -> 'pcd'`` for OSD,
``'depth' -> 'pcd'`` for OCID / HOPE / DoPose) and read with quber_amd.pcd - or, with ``camera=``, from the depth file itself, back-projected
on the device: a ``.npy`` file holds metres, a 16-bit image millimetres (``float32(v) / float32(1000)``: this project's rule; the
reference's only intrinsics branch reads ``.npy``).  The depth must already have the frame's size: there is no float resize here.
cv2 / open3d are absent from the image, so images are read with PIL."""
import os
import time

import numpy as np
import torch
from PIL import Image

from .. import engine as qengine
from ..pcd import read_pcd_xyz

W = 640
H = 480
PCD_RULES = {"OSD": "disparity", "OCID": "depth", "HOPE": "depth", "DoPose": "depth"}


def pcd_path_for(depth_path, dataset):
    """eval/base_model.py:465 / :473; FileNotFoundError when the file is absent, ValueError for a dataset without a rule"""
    if dataset not in PCD_RULES:
        raise ValueError(f"dataset {dataset!r} has no point-cloud files ({sorted(PCD_RULES)} have); pass camera= to use the depth file")
    path = depth_path.replace(PCD_RULES[dataset], "pcd").replace(".png", ".pcd")
    if not os.path.exists(path):
        raise FileNotFoundError("No pcd file found at {0}".format(path))
    return path


def read_depth_metres(depth_path, h, w):
    """-> f32 [h,w] in metres: a .npy file as it is, a 16-bit image as float32(v) / float32(1000)"""
    if depth_path.endswith(".npy"):
        z = np.load(depth_path).astype(np.float32)
    else:
        raw = np.asarray(Image.open(depth_path))
        if raw.ndim != 2 or raw.dtype.kind not in "ui" or raw.dtype.itemsize != 2 and raw.dtype != np.int32:
            raise ValueError(f"{depth_path}: a depth image must be a 16-bit single-channel image (got {raw.dtype} {raw.shape})")
        z = raw.astype(np.float32) / np.float32(1000)
    if z.shape != (h, w):
        raise ValueError(f"{depth_path}: depth of {z.shape} for a frame of {(h, w)}; a float depth is not resized here")
    return np.ascontiguousarray(z)


def load_geometry(depth_path, dataset, camera, h, w):
    """-> ("xyz", f32 [h,w,3]) from the .pcd beside the depth file, or with camera= ("z", f32 [h,w]) from the depth file"""
    if camera is not None:
        return "z", read_depth_metres(depth_path, h, w)
    return "xyz", read_pcd_xyz(pcd_path_for(depth_path, dataset), h, w)


class UOISNet:
    """dsn_weights / rrn_weights: state dicts, checkpoint dicts or paths (or a ready DepthSeeding / RegionRefinement; rrn_weights None:
    the chain ends at the IMP).  camera: a quber_amd.camera.Camera for the frame AS IT IS FED (Camera.scaled for a resized one), or None
    for the .pcd files.  cluster: a GaussianMeanShift, default the reference's uoisnet3d.yaml.  height / width: the frame, multiples of 16."""

    def __init__(self, dsn_weights, rrn_weights, dataset="OCID", camera=None, device="cuda:0", final_close_morphology=False, *,
                 cluster=None, height=H, width=W):
        from ..camera import Camera
        from ..gms import IMP_LDS_BYTES, GaussianMeanShift, imp_plane_bytes
        from ..region import RegionRefinement
        from ..seeding import DepthSeeding
        if camera is not None and not isinstance(camera, Camera):
            raise ValueError(f"camera={camera!r}: expected None or a quber_amd.camera.Camera")
        if camera is None and dataset not in PCD_RULES:
            raise ValueError(f"dataset {dataset!r} has no point-cloud files ({sorted(PCD_RULES)} have); pass camera= to use the depth file")
        if height % 16 or width % 16 or height < 16 or width < 16:
            raise ValueError(f"UOISNet: height and width must be multiples of 16 (got {height} x {width})")
        self.cluster = GaussianMeanShift.uois() if cluster is None else GaussianMeanShift.parse(cluster)
        closes = final_close_morphology or (isinstance(rrn_weights, RegionRefinement) and rrn_weights.final_close_morphology)
        if (self.cluster.imp is not None or closes) and imp_plane_bytes(height, width) > IMP_LDS_BYTES:
            raise ValueError(f"UOISNet: the two bit planes of a {height} x {width} frame do not fit the LDS")
        self.seeding = dsn_weights if isinstance(dsn_weights, DepthSeeding) else DepthSeeding(dsn_weights)
        if rrn_weights is None or isinstance(rrn_weights, RegionRefinement):
            self.region = rrn_weights
        else:
            self.region = RegionRefinement(rrn_weights, final_close_morphology=final_close_morphology)
        self.dataset, self.camera, self.device = dataset, camera, torch.device(device)
        self.H, self.W = height, width
        from ..uois_chain import mask_rows
        qc = qengine.make_config(height, width, max_batch=1, max_instances=max(64, mask_rows(self.cluster, height, width)), with_network=False)
        self.eng = qengine.Engine(qc, self.device)
        self.last = None                                   # the chain's dict of the latest predict (uois_chain)

    def close(self):
        self.eng.close()

    def predict(self, rgb_path, depth_path):
        from ..uois_chain import uois_chain
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        bgr = dev(np.asarray(Image.open(rgb_path).convert("RGB"))[:, :, ::-1])     # BGR like cv2.imread
        if tuple(bgr.shape[:2]) != (self.H, self.W):
            bgr = qengine.resize_u8(bgr, self.H, self.W, linear=True)              # cv2.resize(rgb_img, (640, 480))
        kind, geo = load_geometry(depth_path, self.dataset, self.camera, self.H, self.W)
        start = time.time()
        with torch.cuda.device(self.device):
            x = dev(geo)[None] if kind == "z" else dev(geo).permute(2, 0, 1)[None].contiguous()
            o = uois_chain(self.eng, self.seeding, self.cluster, self.region, bgr[None], x, self.camera)
            ids = (o["region"] if o["region"] is not None else o["cluster"])["ids"][0]
            torch.cuda.synchronize(self.device)
        elapsed = time.time() - start
        self.last = o
        seg = ids.cpu().numpy()
        pred_masks = np.asarray([seg == i for i in np.unique(seg) if i != 0])
        fg_mask = (o["classes"][0] == 2).cpu().numpy()     # 1: table, 2: object
        return pred_masks, fg_mask, elapsed
