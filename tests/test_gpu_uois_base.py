"""GPU: UOIS-Net-3D as a base model - RegionRefinement(final_close_morphology=True) against the numpy IMP contract, and the two adapters that
go from files to masks: quber_amd.eval.base_model.UOISNet and MaskRefiner(seeding=, cluster=, region=[, camera=])."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import golden
from quber_amd import dsn_arch, engine as qengine, rrn_arch
from quber_amd.camera import Camera, xyz_np
from quber_amd.gms import IMP, GaussianMeanShift
from quber_amd.region import RegionRefinement
from quber_amd.seeding import DepthSeeding
from test_gms_cpu import imp_np
from test_pcd_cpu import write_pcd
from test_region_close_cpu import KSIZE, close_np, close_scene, scene_properties
from test_rrn_cpu import rrn_paste_np
from test_zoom_cpu import zoom_rois_np

pytestmark = pytest.mark.gpu

GKW = dict(num_seeds=40, sigma=0.3, epsilon=0.3, min_pixels=100, imp=IMP(5, True), seed=5)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _IdentityNet:
    """stands in for the Region Refinement Network: the refined crop is the mask crop it was given, so the scene decides the shapes"""

    def run(self, rgb, mask, threshold=0.5, logits=True, refined=True, out=None):
        out["refined"].copy_((mask != 0).to(torch.uint8))
        return out


def test_final_close_morphology_scene():
    """the scene of tests/test_region_close_cpu.py through RegionRefinement.refine with the network replaced by the identity (crop, paste and
    close are the real kernels): final_close_morphology=False gives the paste's map, =True the numpy IMP contract (largest component off)
    applied to that map and compacted, bit for bit - ids, masks, source and the report's count and removed ids.  Two frames of a capacity-3
    engine, the second the scene mirrored; properties (a) and (b) are checked on the CPU contract first, on the map the paste really made."""
    ids0 = np.stack([close_scene(), close_scene()[:, ::-1]]).astype(np.int32)
    B, h, w = ids0.shape
    n_ids, S = 6, 64                                                   # more rows than ids: empty rows behind the count
    eng = qengine.Engine(qengine.make_config(h, w, max_batch=3, with_network=False))
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    z = np.broadcast_to(np.float32(1.0), (B, h, w)).copy()
    sd = rrn_arch.init_state_dict(0, gain=0.7, feature_dim=8)
    counts = [4, 4]
    res = {}
    for close in (False, True):
        region = RegionRefinement(sd, padding=0.0, crop=S, chunk=3, final_close_morphology=close, ksize=KSIZE)
        region._engines[(region.crop, region.chunk, str(eng.device))] = _IdentityNet()
        res[close] = {k: v.cpu().numpy() for k, v in region.refine(eng, _dev(img), _dev(ids0), n_ids, counts, _dev(z)).items()}
    off, on = res[False], res[True]
    # =False: the parent's map - the paste contract on the refined crops the call itself made
    slots = np.array([(b, i) for b in range(B) for i in range(1, 5)], np.int32)
    rois = zoom_rois_np(ids0, n_ids, 0.0)
    assert np.array_equal(off["rois"], rois) and np.array_equal(off["slots"], slots)
    want = rrn_paste_np(off["refined"], slots, rois, z, B, h, w, n_ids)
    for k in ("ids", "masks", "source", "report"):
        assert np.array_equal(off[k], want[k]), k
    assert off["report"].shape == (B, 4) and on["report"].shape == (B, 5)
    for b in range(B):
        before = off["ids"][b]
        assert before.max() == 4
        scene_properties(before)                                       # (a) an id vanishes and the rest shift, (b) the later closing wins
        closed, report, keep = imp_np(before, n_ids, KSIZE, largest=False)
        assert np.array_equal(closed, close_np(before, n_ids)[0])
        assert np.array_equal(on["ids"][b], closed), "frame %d: ids" % b
        assert int(closed.max()) == 3 and keep == [2, 3, 4] and report.tolist() == [3, 1]
        for j in range(n_ids):
            assert np.array_equal(on["masks"][b, j], np.where(closed == j + 1, 255, 0).astype(np.uint8)), "frame %d: mask %d" % (b, j)
        assert on["source"][b].tolist() == [2, 3, 4, 0, 0, 0], on["source"][b].tolist()
        assert on["report"][b].tolist() == [3, int(off["report"][b, 1]), int(off["report"][b, 2]), int(off["report"][b, 3]), 1]
        assert not np.array_equal(on["ids"][b], before)
    eng.close()


def _frames(h, w):
    from quber_amd import synth
    sc = [synth.make_scene(3 + b, h, w, 2) for b in range(2)]
    return np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])


def test_predict_final_close_morphology():
    """the predictor with region=RegionRefinement(final_close_morphology=True) and the real networks: region_ids equal the numpy IMP contract
    applied to the region_ids of the same predictor with =False (which are the parent's: tests/test_gpu_rrn.py holds them), region_masks /
    region_source / region_report follow, the cluster_* entries keep the masks before the network, and the refiner encodes the closed masks."""
    from test_gpu_cleanup import speck_logits
    from test_gpu_masknms import _equal, _predictor
    f = np.load([p for p in golden("dsn_scene") if "96x128" in p][0])
    h, w = f["xyz"].shape[1:]
    rgb, dep = _frames(h, w)
    seeding = DepthSeeding(dsn_arch.init_state_dict(int(f["seed"]), gain=float(f["gain"])))
    rsd = rrn_arch.init_state_dict(0, gain=0.7, feature_dim=8)
    outs, offs, preds, regions = {}, {}, [], []
    for close in (False, True):
        region = RegionRefinement(rsd, threshold=0.3, crop=32, chunk=3, final_close_morphology=close, ksize=3)
        offs[close] = []
        p = _predictor(h, w, speck_logits(h, w), offs[close], cluster=GaussianMeanShift(**GKW), seeding=seeding, region=region, track_initial=True)
        outs[close] = p.predict(rgb[0], dep[0], xyz=f["xyz"])[0]
        preds.append(p)
        regions.append(region)
    a, b = outs[True], outs[False]
    assert set(a) == set(b)
    for key in [k for k in b if k.startswith(("cluster_", "seeding_"))] + ["region_rois"]:
        _equal(a[key], b[key], key)
    before = b["region_ids"].cpu().numpy()
    n = b["cluster_masks"].shape[0]
    want, report, keep = imp_np(before, n, 3, largest=False)                # (seeded weights: the refined masks are ragged, a wider ellipse removes them all)
    print("region ids before %d, after %d, removed %d" % (before.max(), want.max(), report[1]))
    assert before.max() >= 1, "no refined mask: the comparison is empty"
    assert np.array_equal(a["region_ids"].cpu().numpy(), want)
    k = int(report[0])
    assert a["region_masks"].shape[0] == k
    for j in range(k):
        assert np.array_equal(a["region_masks"][j].cpu().numpy(), np.where(want == j + 1, 255, 0).astype(np.uint8))
    assert a["region_source"].tolist() == [b["region_source"].tolist()[o - 1] for o in keep]
    assert a["region_report"].tolist() == [k] + b["region_report"].tolist()[1:4] + [int(report[1])] and len(b["region_report"]) == 4
    eng = preds[1].model.engine_for(h, w, 1, n)
    m = np.zeros((1, n, h, w), np.uint8)
    m[0, :k] = a["region_masks"].cpu().numpy()
    assert torch.equal(offs[True][-1], eng.encode(_dev(m)))
    seeding.close()
    for r in regions:
        r.close()
    for p in preds:
        p.model.close()


def _save_png(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)
    return str(path)


def test_uoisnet_predict_from_files(tmp_path):
    """UOISNet.predict on files the test writes: png + ascii pcd (the 'depth' -> 'pcd' rule), and png of twice the size + .npy depth with camera=
    (the resize and the device back-projection).  Masks = the np.unique-ordered masks of the predictor chain's region map on the same frame,
    fg_mask = class 2; with final_close_morphology the closed map; the refusals."""
    from quber_amd.eval.base_model import UOISNet
    from test_gpu_cleanup import speck_logits
    from test_gpu_masknms import _predictor
    f = np.load([p for p in golden("dsn_scene") if "96x128" in p][0])
    h, w = f["xyz"].shape[1:]
    rgb, dep = _frames(h, w)
    seeding = DepthSeeding(dsn_arch.init_state_dict(int(f["seed"]), gain=float(f["gain"])))
    rsd = rrn_arch.init_state_dict(0, gain=0.7, feature_dim=8)
    region = RegionRefinement(rsd, crop=32, chunk=3)
    cam = Camera(118.0, 121.0, 63.5, 47.25)
    z = np.ascontiguousarray(f["xyz"][2])
    xyz_file = np.ascontiguousarray(f["xyz"].transpose(1, 2, 0))       # [h,w,3], NaN where there is no depth

    def chain(bgr, **kw):
        """the predictor chain on the same frame, a fresh clustering stream"""
        p = _predictor(h, w, speck_logits(h, w), [], cluster=GaussianMeanShift(**GKW), seeding=seeding, region=region)
        o = p.predict(bgr, dep[0], **kw)[0]
        ids, cls = o["region_ids"].cpu().numpy(), o["seeding_fg"].cpu().numpy()
        p.model.close()
        return ids, cls

    # -- png + ascii pcd, frame size as it is --
    rgb_path = _save_png(str(tmp_path / "rgb" / "a.png"), rgb[0])
    depth_path = _save_png(str(tmp_path / "depth" / "a.png"), np.nan_to_num(z * 1000).astype(np.uint16))
    os.makedirs(tmp_path / "pcd")
    write_pcd(tmp_path / "pcd" / "a.pcd", xyz_file.reshape(-1, 3), "ascii", ("x", "y", "z", "rgb"), width=w, height=h)
    net = UOISNet(seeding, region, dataset="OCID", cluster=GaussianMeanShift(**GKW), height=h, width=w)
    masks, fg, seconds = net.predict(rgb_path, depth_path)
    bgr = np.ascontiguousarray(rgb[0][:, :, ::-1])                      # cv2.imread's order of the file's pixels
    ids, cls = chain(bgr, xyz=xyz_file)
    want = np.asarray([ids == i for i in np.unique(ids) if i != 0])
    print("pcd: %d masks, %d object pixels, %.1f ms" % (len(want), int((cls == 2).sum()), seconds * 1e3))
    assert len(want) >= 1, "no mask: the comparison is empty"
    assert masks.dtype == np.bool_ and masks.shape == want.shape and np.array_equal(masks, want)
    assert fg.dtype == np.bool_ and np.array_equal(fg, cls == 2) and seconds > 0
    with pytest.raises(FileNotFoundError):
        net.predict(rgb_path, str(tmp_path / "depth" / "b.png"))
    net.close()
    # -- OSD's rule --
    os.makedirs(tmp_path / "disparity")
    osd = UOISNet(seeding, region, dataset="OSD", cluster=GaussianMeanShift(**GKW), height=h, width=w)
    with pytest.raises(FileNotFoundError):
        osd.predict(rgb_path, depth_path)                              # 'depth/a.png' holds no 'disparity'
    m2 = osd.predict(rgb_path, str(tmp_path / "disparity" / "a.png"))[0]
    assert np.array_equal(m2, want)
    osd.close()
    # -- a png of twice the size + .npy metres with camera=, final close on --
    big = np.ascontiguousarray(np.repeat(np.repeat(rgb[1], 2, 0), 2, 1))
    big[::2, 1::2] //= 2                                                # (not a plain doubling: the linear resize has something to do)
    rgb2 = _save_png(str(tmp_path / "rgb" / "c.png"), big)
    npy = str(tmp_path / "depth" / "c.npy")
    np.save(npy, z)
    closing = RegionRefinement(rsd, crop=32, chunk=3, final_close_morphology=True, ksize=3)
    net = UOISNet(seeding, closing, dataset="WISDOM", camera=cam, cluster=GaussianMeanShift(**GKW), height=h, width=w)
    masks, fg, _ = net.predict(rgb2, npy)
    small = qengine.resize_u8(_dev(np.ascontiguousarray(big[:, :, ::-1])), h, w, True).cpu().numpy()
    ids, cls = chain(small, xyz=xyz_np(z, cam))
    closed = imp_np(ids, int(ids.max()), 3, largest=False)[0]
    want = np.asarray([closed == i for i in np.unique(closed) if i != 0])
    print("camera: %d masks before the close, %d after" % (int(ids.max()), len(want)))
    assert ids.max() >= 1 and masks.shape == want.shape and np.array_equal(masks, want)
    assert np.array_equal(fg, cls == 2)
    # a 16-bit image is millimetres: float32(v) / float32(1000)
    mm = np.nan_to_num(z * 1000).astype(np.uint16)
    png16 = _save_png(str(tmp_path / "depth" / "d.png"), mm)
    net.cluster.reseed()                                                # (the object owns its stream of draws: the chain below starts a fresh one)
    masks16 = net.predict(rgb2, png16)[0]
    ids16, _ = chain(small, xyz=xyz_np(mm.astype(np.float32) / np.float32(1000), cam))
    closed16 = imp_np(ids16, int(ids16.max()), 3, largest=False)[0]
    assert np.array_equal(masks16, np.asarray([closed16 == i for i in np.unique(closed16) if i != 0]))
    np.save(str(tmp_path / "depth" / "e.npy"), z[:, :-1])
    with pytest.raises(ValueError):
        net.predict(rgb2, str(tmp_path / "depth" / "e.npy"))            # another size: no float resize here
    net.close()
    for bad in (lambda: UOISNet(seeding, region, dataset="WISDOM"), lambda: UOISNet(seeding, region, camera=(1, 1, 0, 0)),
                lambda: UOISNet(seeding, region, height=50, width=80)):
        with pytest.raises(ValueError):
            bad()
    seeding.close()
    region.close()
    closing.close()


def test_maskrefiner_adapter_runs_the_chain(tmp_path):
    """MaskRefiner(seeding=, cluster=, region=).predict(rgb_path, depth_path) = predict(rgb_path, depth_path, initial_masks=its region_masks) on
    an adapter without the base-model arguments: the same refined masks and semantic logits.  camera= with the depth file gives the masks of the
    contract's point cloud; the refusals."""
    from quber_amd.eval.refiner_model import H, W, MaskRefiner
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:H, 0:W]
    z = (0.9 + 0.0004 * yy + 0.0002 * xx).astype(np.float32)
    for k, (cy, cx) in enumerate(((150, 200), (300, 420), (330, 150))):
        z[(yy - cy) ** 2 + (xx - cx) ** 2 < (50 + 10 * k) ** 2] -= np.float32(0.15 + 0.05 * k)
    z[10:20, 30:60] = np.nan
    cam = Camera(570.3, 570.3, 319.5, 239.5)
    xyz = xyz_np(z, cam)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb_path = _save_png(str(tmp_path / "rgb" / "f.png"), rgb)
    depth_path = _save_png(str(tmp_path / "disparity" / "f.png"), np.nan_to_num(z * 1000).astype(np.uint16))
    os.makedirs(tmp_path / "pcd")
    write_pcd(tmp_path / "pcd" / "f.pcd", xyz.reshape(-1, 3), "binary", ("x", "y", "z", "rgb"), width=W, height=H)
    gkw = dict(GKW, min_pixels=300, imp=IMP(9, True))
    seeding = DepthSeeding(dsn_arch.init_state_dict(3, gain=0.7, feature_dim=8))
    region = RegionRefinement(rrn_arch.init_state_dict(0, gain=0.7, feature_dim=8), crop=32, chunk=8)
    base = MaskRefiner(dataset="OSD", seeding=seeding, cluster=GaussianMeanShift(**gkw), region=region, camera=cam)
    plain = MaskRefiner(dataset="OSD")
    pred = base.refiner_predictor
    # camera=: the depth file itself; 16-bit millimetres
    out3 = base.predict(rgb_path, depth_path)[1]
    mm = np.nan_to_num(z * 1000).astype(np.uint16).astype(np.float32) / np.float32(1000)
    pred.cluster.reseed()
    fr = base._load(rgb_path, depth_path, np.zeros((0, H, W), np.uint8))
    out4 = pred.predict(fr["rgb"], fr["depth"], xyz=xyz_np(mm, cam))[0]
    assert torch.equal(out3["region_ids"], out4["region_ids"]) and torch.equal(out3["seeding_fg"], out4["seeding_fg"])
    # without it (the attribute is what predict reads; a second adapter would build the refiner a third time): the .pcd beside the depth file
    base.camera = None
    pred.cluster.reseed()
    refined, out, seconds, _ = base.predict(rgb_path, depth_path)
    init = out["region_masks"].cpu().numpy()
    print("adapter: %d clusters, %d refined initial masks, %d instances" % (int(out["cluster_report"][0]), len(init), len(refined)))
    assert {"cluster_masks", "cluster_ids", "region_masks", "region_ids", "seeding_fg"} <= set(out) and seconds > 0
    refined2, out2, _, _ = plain.predict(rgb_path, depth_path, initial_masks=init)
    assert np.array_equal(np.asarray(refined), np.asarray(refined2))
    assert torch.equal(out["sem_seg"], out2["sem_seg"])
    for bad in (lambda: plain.predict(rgb_path, depth_path), lambda: base.predict(rgb_path, depth_path, initial_masks=init),
                lambda: next(iter(base.predict_stream([(rgb_path, depth_path, init)]))), lambda: MaskRefiner(dataset="OSD", camera=cam),
                lambda: MaskRefiner(dataset="armbench", seeding=seeding, cluster=GaussianMeanShift(**gkw))):
        with pytest.raises(ValueError):
            bad()
    lone = _save_png(str(tmp_path / "disparity" / "g.png"), np.nan_to_num(z * 1000).astype(np.uint16))
    with pytest.raises(FileNotFoundError):
        base.predict(rgb_path, lone)                                   # a depth file without a .pcd beside it
    seeding.close()
    region.close()
    for m in (base, plain):
        m.refiner_predictor.model.close()
