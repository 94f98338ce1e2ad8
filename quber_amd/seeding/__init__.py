"""The Depth Seeding Network of UOIS-Net-3D on the MI355X HIP path (csrc/dsn.hip, csrc/plan_dsn.hip): xyz -> foreground logits, centre
offsets, centre votes and the foreground map that ``cluster=GaussianMeanShift()`` reads, without leaving the device.

``DsnEngine`` is one context for a fixed frame size and batch capacity; ``DepthSeeding`` the options object of
``MaskRefinerPredictor(..., cluster=GaussianMeanShift.uois(), seeding=DepthSeeding(weights))``."""
import ctypes as C

import numpy as np
import torch

from .. import _lib, dsn_arch, engine as qengine

DSN_FUSED = 53                 # option key: the second half of an ESP module as one kernel (csrc/dsn.hip esp_branches) or from separate launchers
NEGATE_Y = 1                   # bit 0 of quber_dsn_forward's flags


class DsnEngine:
    """One Depth Seeding Network context (quber_config.with_network = 4).  h and w must be multiples of 16.  fused: option key 53, None =
    the library's default.  All methods are asynchronous on torch's current stream and take device tensors."""

    def __init__(self, state_dict, h=480, w=640, max_batch=1, fused=None, device="cuda:0", negate_y=True):
        if h % 16 or w % 16 or h < 16 or w < 16:
            raise ValueError(f"DsnEngine: height and width must be multiples of 16 (got {h} x {w})")
        sd = dsn_arch.load_checkpoint(state_dict)
        self.feature_dim = int(sd["encoder.layer1.layer1.conv1.weight"].shape[0])
        qc = qengine.make_config(h, w, max_batch=max_batch)
        qc.with_network = 4
        self.eng = qengine.Engine(qc, device)
        if fused is not None:
            self.eng.set_option(DSN_FUSED, int(bool(fused)))
        # the context's inventory names the keys; the sizes follow from feature_dim, which the plan reads off the first convolution
        lib = self.eng.lib
        for name, _ in self.eng.weight_specs():
            v = sd[name]
            _lib.check(lib.quber_set_weight(self.eng.h, name.encode(), C.c_void_p(v.ctypes.data), v.size))
        with torch.cuda.device(self.eng.device):
            _lib.check(lib.quber_finalize_weights(self.eng.h))
        self.device = self.eng.device
        self.H, self.W, self.max_batch = h, w, max_batch
        self.flags = NEGATE_Y if negate_y else 0

    def close(self):
        self.eng.close()

    def _check(self, xyz):
        B = xyz.shape[0]
        if not (xyz.dtype == torch.float32 and xyz.is_contiguous() and xyz.is_cuda and tuple(xyz.shape) == (B, 3, self.H, self.W)):
            raise ValueError(f"DsnEngine: xyz must be a contiguous float32 device tensor [B,3,{self.H},{self.W}]")
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"DsnEngine: batch {B} outside 1..{self.max_batch}")
        return B

    def _check_z(self, xyz, z, camera):
        """the depth form of a call: z f32 [B,H,W] on the device (metres) and a quber_amd.camera.Camera -> (B, its four doubles)"""
        from ..camera import Camera
        if xyz is not None or z is None or camera is None:
            raise ValueError("DsnEngine: either xyz, or z= together with camera=")
        if not isinstance(camera, Camera):
            raise ValueError(f"DsnEngine: camera={camera!r}, expected a quber_amd.camera.Camera")
        B = z.shape[0] if isinstance(z, torch.Tensor) and z.dim() else 0
        if not (isinstance(z, torch.Tensor) and z.dtype == torch.float32 and z.is_contiguous() and z.is_cuda and tuple(z.shape) == (B, self.H, self.W)):
            raise ValueError(f"DsnEngine: z must be a contiguous float32 device tensor [B,{self.H},{self.W}]")
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"DsnEngine: batch {B} outside 1..{self.max_batch}")
        return B, (C.c_double * 4)(*camera.params)

    def run(self, xyz=None, logits=False, offsets=False, votes=False, classes=False, fg=False, z=None, camera=None):
        """xyz f32 [B,3,H,W] (planar x, y, z; NaN allowed) - or z= f32 [B,H,W] (metres) with camera= (a quber_amd.camera.Camera): the plan's
        first op then back-projects and packs in one kernel - -> dict of the requested outputs: "fg_logits" / "center_offsets" / "votes" f32
        [B,3,H,W], "fg_classes" / "fg" u8 [B,H,W]."""
        cam = None
        if z is not None or camera is not None:
            B, cam = self._check_z(xyz, z, camera)
        else:
            B = self._check(xyz)
        new = lambda want, c, dt: torch.empty((B, 3, self.H, self.W) if c else (B, self.H, self.W), dtype=dt, device=self.device) if want else None
        o = {"fg_logits": new(logits, 1, torch.float32), "center_offsets": new(offsets, 1, torch.float32), "votes": new(votes, 1, torch.float32),
             "fg_classes": new(classes, 0, torch.uint8), "fg": new(fg, 0, torch.uint8)}
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        outs = (p(o["fg_logits"]), p(o["center_offsets"]), p(o["votes"]), p(o["fg_classes"]), p(o["fg"]), st)
        with torch.cuda.device(self.device):
            if cam is None:
                _lib.check(self.eng.lib.quber_dsn_forward(self.eng.h, p(xyz), B, self.flags, *outs))
            else:
                _lib.check(self.eng.lib.quber_dsn_forward_depth(self.eng.h, p(z), B, self.flags, cam, camera.convention_id, *outs))
        return {k: v for k, v in o.items() if v is not None}

    def profile(self, xyz=None, z=None, camera=None):
        """One forward with an event pair around every op -> [(op name, ms)] in plan order; synchronises (tools/dsn_ab.py, tools/xyz_ab.py)."""
        cam = None
        if z is not None or camera is not None:
            B, cam = self._check_z(xyz, z, camera)
        else:
            B = self._check(xyz)
        plan = self.eng.plan()
        ms = (C.c_double * len(plan))()
        cls = torch.empty((B, self.H, self.W), dtype=torch.uint8, device=self.device)
        tail = (None, None, None, C.c_void_p(cls.data_ptr()), None, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), ms)
        with torch.cuda.device(self.device):
            if cam is None:
                _lib.check(self.eng.lib.quber_dsn_forward_profiled(self.eng.h, C.c_void_p(xyz.data_ptr()), B, self.flags, *tail))
            else:
                _lib.check(self.eng.lib.quber_dsn_forward_depth_profiled(self.eng.h, C.c_void_p(z.data_ptr()), B, self.flags, cam, camera.convention_id, *tail))
        return [(p[0], ms[i]) for i, p in enumerate(plan)]

    def forward(self, xyz=None, z=None, camera=None):
        """-> (fg_logits, center_offsets), f32 [B,3,H,W] each: DepthSeedingNetwork.forward on the cleaned input"""
        o = self.run(xyz, logits=True, offsets=True, z=z, camera=camera)
        return o["fg_logits"], o["center_offsets"]

    def seed(self, xyz=None, z=None, camera=None):
        """-> (votes f32 [B,3,H,W] = cleaned xyz + offsets, fg u8 [B,H,W] = (class == 2), fg_classes u8 [B,H,W] in 0 / 1 / 2): what
        Engine.gms reads, and the reference's fg_mask"""
        o = self.run(xyz, votes=True, classes=True, fg=True, z=z, camera=camera)
        return o["votes"], o["fg"], o["fg_classes"]


class DepthSeeding:
    """Options of ``MaskRefinerPredictor(seeding=...)``: the weights (a state dict, a checkpoint dict with it under 'model', or a path to
    one; DataParallel's ``module.`` prefix is stripped) and whether y is negated on the way in (eval/base_model.py:498; the reference
    always does).  fused: option key 53, None = the library's default."""

    def __init__(self, weights_or_path, negate_y=True, fused=None):
        self.state_dict = dsn_arch.load_checkpoint(weights_or_path)
        self.negate_y = bool(negate_y)
        self.fused = fused
        self._engines = {}

    def engine_for(self, h, w, max_batch, device):
        key = (h, w, max_batch, str(device))
        if key not in self._engines:
            self._engines[key] = DsnEngine(self.state_dict, h, w, max_batch, fused=self.fused, device=device, negate_y=self.negate_y)
        return self._engines[key]

    def close(self):
        for e in self._engines.values():
            e.close()
        self._engines = {}


def as_xyz_batch(xyz, h, w, device):
    """one [h,w,3] / [3,h,w] array or tensor, or a list of them -> contiguous f32 device tensor [B,3,h,w] (the reference's xyz images are
    [h,w,3]: base_model.py:494)"""
    items = xyz if isinstance(xyz, (list, tuple)) else [xyz]
    out = []
    for a in items:
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dim() != 3 or (tuple(t.shape) != (3, h, w) and tuple(t.shape) != (h, w, 3)):
            raise ValueError(f"xyz: expected [{h},{w},3] or [3,{h},{w}], got {tuple(t.shape)}")
        if tuple(t.shape) != (3, h, w):
            t = t.permute(2, 0, 1)
        out.append(t.to(device=device, dtype=torch.float32))
    return torch.stack(out).contiguous()
