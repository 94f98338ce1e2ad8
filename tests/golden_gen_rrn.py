"""Generator of tests/golden/rrn_net_*.npz and tests/golden/rrn_scene_*.npz.  Not collected by pytest; run by hand on a CPU machine that
has the reference:

    python tests/golden_gen_rrn.py --reference /path/to/reference/ext_modules

It imports the reference's uois/src/segmentation.py by path (torch only; an empty stand-in is registered for ``cv2``, the one import that
may be missing and that nothing used here touches).  Only data are written.

rrn_net_{S}.npz, S = 32 and 48: RegionRefinementNetwork(UNet_Encoder(4, 64), UNet_Decoder(1, 64), 1x1 head) with
rrn_arch.init_state_dict(seed, gain) loaded strict=True, run in float32 and float64 on two rrn_torch.synth_crops: the seed and gain (the
weights are regenerated from them), the crops, the float32 logits, the key names and shapes of the module's state_dict, and
    ref_f32_err      max |reference float32 - reference float64|
    near_zero_share  share of pixels with |float64 logit| < 2e-4
    mask_share       share of positive pixels
The first (seed, gain) of the search order with ref_f32_err <= 2.5e-5, near_zero_share < 5e-4 and mask_share in 5-95 % on BOTH fixtures is
taken, and the conditions are asserted: the GPU test's 1e-4 and its 99.9 % mask agreement rest on them.

rrn_scene_{h}x{w}.npz: UOISNet3D.rrn_preprocess / rrn_postprocess, called unbound on a stand-in for self, with S = 32: the reference writes
its crop side 224 as a literal, so its calls of torch.zeros, F.upsample_bilinear and F.upsample_nearest go through stand-ins that replace a
224 by S and do nothing else.  Inputs: the frame's bytes, an id map over {0, 2, 3, 5, 6} (a one-pixel mask in a corner, one touching two
borders, one whose ROI is wider than S and lower, one whose ROI overlaps it), a z plane, synthetic refined crops (none empty: a NaN mean
leaves the reference's own sort undefined).  Recorded: crop_indices, the rgb and mask crops, the painted map.  Asserted: any two mean
depths differ by more than 1e-3 of the largest |z|, far above the float32 error of a mean, so the paint order is unambiguous."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rrn_torch as R                                    # noqa: E402
from quber_amd import rrn_arch                           # noqa: E402
from quber_amd.region import standardize_table           # noqa: E402

NET_SIZES = ((32, 51), (48, 52))                         # crop side, crop seed
SCENES = ((48, 64, 61), (96, 128, 62))                   # h, w, seed
S_SCENE = 32
MAX_F32_ERR, MAX_ZERO_SHARE, NEAR, FD = 2.5e-5, 5e-4, 2e-4, 64


def reference_segmentation(ref_dir):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    pkg = types.ModuleType("reference_uois_src")
    pkg.__path__ = [os.path.join(ref_dir, "uois", "src")]
    sys.modules["reference_uois_src"] = pkg
    spec = importlib.util.spec_from_file_location("reference_uois_src.segmentation", os.path.join(ref_dir, "uois", "src", "segmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_uois_src.segmentation"] = mod
    spec.loader.exec_module(mod)
    return mod


def make_net(seg):
    nets = seg.networks
    return seg.RegionRefinementNetwork(nets.UNet_Encoder(input_channels=4, feature_dim=FD), nets.UNet_Decoder(num_encoders=1, feature_dim=FD),
                                       torch.nn.Conv2d(FD, 1, kernel_size=1, stride=1, padding=0, bias=False))


def evaluate_net(seg, seed, gain):
    sd = rrn_arch.init_state_dict(seed, gain=gain, feature_dim=FD)
    net = make_net(seg).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert keys == [(k, tuple(s)) for k, (s, _) in rrn_arch.param_specs(FD).items()], "param_specs differs from the module"
    assert sum(v.numel() for v in net.state_dict().values()) == rrn_arch.N_PARAMS_FD64
    net64 = make_net(seg).eval().double()
    net64.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=True)
    out = []
    for S, cs in NET_SIZES:
        rgb, mask = R.synth_crops(2, S, cs)
        tr, tm = torch.from_numpy(rgb), torch.from_numpy(mask).float()
        with torch.no_grad():
            l32 = net({"rgb": tr, "initial_masks": tm})
            l64 = net64({"rgb": tr.double(), "initial_masks": tm.double()})
        out.append(dict(S=S, rgb=rgb, mask=mask, logits=l32.numpy(), err=float((l32.double() - l64).abs().max()),
                        zero=float((l64.abs() < NEAR).double().mean()), share=float((l64 > 0).double().mean()), keys=keys, span=float(l64.abs().max())))
    return out


def good(r):
    return r["err"] <= MAX_F32_ERR and r["zero"] < MAX_ZERO_SHARE and 0.05 < r["share"] < 0.95


def write_nets(seg, out_dir):
    chosen = None
    for gain in (0.7, 0.8, 0.6, 0.5, 1.0):
        for seed in range(8):
            res = evaluate_net(seg, seed, gain)
            print("seed %d gain %.2f: " % (seed, gain) + "; ".join(
                "S %d err %.2e near-zero %.1e max|logit| %.2f positive %.3f" % (r["S"], r["err"], r["zero"], r["span"], r["share"]) for r in res), flush=True)
            if all(good(r) for r in res):
                chosen = (seed, gain, res)
                break
        if chosen:
            break
    assert chosen, "no (seed, gain) of the search order meets the conditions"
    seed, gain, res = chosen
    for r in res:
        assert good(r)
        path = os.path.join(out_dir, "rrn_net_%d.npz" % r["S"])
        np.savez_compressed(path, seed=np.int64(seed), gain=np.float64(gain), feature_dim=np.int64(FD), rgb=r["rgb"], mask=r["mask"], logits=r["logits"],
                            keys=np.array([k for k, _ in r["keys"]]), shapes=np.array([list(s) + [0] * (4 - len(s)) for _, s in r["keys"]], np.int32),
                            ref_f32_err=np.float64(r["err"]), near_zero_share=np.float64(r["zero"]), mask_share=np.float64(r["share"]))
        size = os.path.getsize(path)
        assert size < 1000000, (path, size)
        print("wrote %s (%d bytes): seed %d gain %.2f ref_f32_err %.3e near_zero_share %.2e mask_share %.3f" % (path, size, seed, gain, r["err"], r["zero"], r["share"]))


class _Swap:
    """a module namespace in which a literal 224 of the named calls' size argument reads S"""

    def __init__(self, real, names, S):
        self._real, self._names, self._S = real, names, S

    def __getattr__(self, k):
        f = getattr(self._real, k)
        if k not in self._names:
            return f
        sub = lambda a: tuple(self._S if v == 224 else v for v in a) if isinstance(a, tuple) else a
        return lambda *args, **kw: f(*[sub(a) for a in args], **kw)


def make_scene(h, w, seed):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[..., 0] = (0.5 * img[..., 0] + 0.5 * (255.0 * xs / w)).astype(np.uint8)
    ids = np.zeros((h, w), np.int32)
    ids[0, 0] = 2                                                                    # one pixel in a frame corner: a 1 x 1 ROI
    ids[(ys > h - h // 3) & (xs > w - w // 4) & ((ys + xs) % 7 != 0)] = 3             # touches two borders
    y0, x0 = h // 4, w // 8
    ids[y0:y0 + 10, x0:x0 + 40] = 5                                                  # ROI wider than S = 32 and lower
    ids[y0 + 6:y0 + 6 + h // 3, x0 + 30:x0 + 44][ids[y0 + 6:y0 + 6 + h // 3, x0 + 30:x0 + 44] == 0] = 6    # its ROI overlaps that of 5
    z = (1.0 + 0.05 * ys / h + 0.03 * xs / w + rng.normal(0, 0.003, (h, w))).astype(np.float32)
    for i, d in ((3, -0.31), (5, 0.25), (6, -0.15)):
        z[ids == i] += np.float32(d)
    z[h // 2, w // 2] = np.nan
    return img, ids, z


def write_scenes(seg, out_dir):
    S = S_SCENE
    table = standardize_table()
    for h, w, seed in SCENES:
        img, ids, z = make_scene(h, w, seed)
        std = np.stack([table[c][img[..., c]] for c in range(3)])                    # standardize_image, [3,h,w]
        me = types.SimpleNamespace(device=torch.device("cpu"), config={"padding_percentage": 0.25})
        seg.torch, seg.F = _Swap(torch, ("zeros",), S), _Swap(torch.nn.functional, ("upsample_bilinear", "upsample_nearest"), S)
        try:
            batch, crop_indices = seg.UOISNet3D.rrn_preprocess(me, torch.from_numpy(std), torch.from_numpy(ids))
        finally:
            seg.torch, seg.F = torch, torch.nn.functional
        mask_ids = sorted(crop_indices)
        assert mask_ids == [2, 3, 5, 6] and list(crop_indices) == mask_ids
        n = len(mask_ids)
        rng = np.random.default_rng(seed + 1)
        yy, xx = np.mgrid[0:S, 0:S] / S
        refined = np.zeros((n, S, S), np.uint8)
        for i in range(n):
            cy, cx, ry, rx = rng.uniform(0.4, 0.6), rng.uniform(0.4, 0.6), rng.uniform(0.3, 0.6), rng.uniform(0.3, 0.6)
            refined[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.uint8)
        refined[0] = 1                                                                # the 1 x 1 ROI keeps its pixel
        assert all(refined[i].any() for i in range(n))
        zc = np.where(np.isnan(z), np.float32(0), z)
        xyz = torch.from_numpy(np.stack([np.zeros_like(zc), np.zeros_like(zc), zc]))
        painted = seg.UOISNet3D.rrn_postprocess(me, torch.from_numpy(refined), crop_indices, xyz).numpy().astype(np.int32)
        means = []
        for i, m in enumerate(mask_ids):
            x0, y0, x1, y1 = crop_indices[m]
            rm = torch.nn.functional.upsample_nearest(torch.from_numpy(refined[i])[None, None].float(), (y1 - y0 + 1, x1 - x0 + 1))[0, 0].numpy() > 0
            assert rm.any()
            means.append(float(zc[y0:y1 + 1, x0:x1 + 1][rm].astype(np.float64).mean()))
        gap = min(abs(a - b) for i, a in enumerate(means) for b in means[i + 1:])
        assert gap > 1e-3 * float(np.abs(zc).max()), (means, gap)
        assert len(np.unique(painted)) >= 4, "a mask vanished under the others: the scene would not show the paint order"
        path = os.path.join(out_dir, "rrn_scene_%dx%d.npz" % (h, w))
        np.savez_compressed(path, img=img, ids=ids, z=z, S=np.int64(S), padding=np.float64(0.25), mask_ids=np.array(mask_ids, np.int32),
                            crop_indices=np.array([[int(v) for v in crop_indices[m]] for m in mask_ids], np.int32), refined=refined,
                            rgb_crops=batch["rgb"].numpy().astype(np.float32), mask_crops=batch["initial_masks"].numpy().astype(np.uint8), painted=painted,
                            mean_depths=np.array(means))
        size = os.path.getsize(path)
        assert size < 1000000, (path, size)
        print("wrote %s (%d bytes): ids %s rois %s mean depths %s" % (path, size, mask_ids, [[int(v) for v in crop_indices[m]] for m in mask_ids], ["%.4f" % m for m in means]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the directory that holds uois/src/segmentation.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", choices=("nets", "scenes"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    seg = reference_segmentation(a.reference)
    if a.only != "nets":
        write_scenes(seg, a.out)
    if a.only != "scenes":
        write_nets(seg, a.out)


if __name__ == "__main__":
    main()
