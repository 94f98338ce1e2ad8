"""GPU: depth -> organised point cloud on the device (csrc/dsn.hip xyz_from_depth_kernel) against the numpy contract quber_amd.camera.xyz_np,
bit for bit, stand-alone (quber_op_xyz_from_depth) and as the first op of the Depth Seeding Network's plan (quber_dsn_forward_depth);
then camera= / depth_z= through MaskRefinerPredictor against the xyz= call on the contract's point cloud, entry by entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
from quber_amd import _lib, dsn_arch, rrn_arch
from quber_amd.camera import Camera, xyz_np
from quber_amd.seeding import DepthSeeding, DsnEngine
from test_xyz_cpu import same_bits, special_depth

pytestmark = pytest.mark.gpu

CAMS = {"pinhole": Camera(1105.0, 1105.0, 511.5, 384.0).scaled(1032, 772, 80, 48),
        "uois": Camera(61.7 + 0.13 * 80, 59.3 + 0.11 * 48, 80 / 2 - 0.37, 48 / 2 + 0.21, "uois")}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cam4(cam):
    return (C.c_double * 4)(*cam.params)


def depth_batch(B, h, w, seed):
    """B frames of special_depth (0, NaN, negative, near the float32 maximum, inf, a denormal among metres); 48 x 80: frame 0 is the z of
    the Depth Seeding Network's scene fixture"""
    z = np.stack([special_depth(h, w, seed + b) for b in range(B)])
    if (h, w) == (48, 80):
        z[0] = np.load([p for p in golden("dsn_scene") if "48x80" in p][0])["xyz"][2]
    return z


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("convention", ["pinhole", "uois"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 5), (3, 48, 80)], ids=["1x1", "3x5", "3x48x80"])
def test_xyz_from_depth_op(shape, convention, flags):
    """all three outputs against xyz_np; x8 / clean also against quber_op_dsn_pack applied to the raw planes the op itself wrote.  1 x 1: the
    flipped row index is 0; 3 x 5: an odd width, no multiple-of-16 rule; 3 x 48 x 80: more than one block, frames after the first."""
    lib = _lib.load()
    B, h, w = shape
    cam = CAMS[convention]
    z = depth_batch(B, h, w, 11)
    if h * w > 1:
        assert np.isnan(z).any() and (z == 0).any() and (z < 0).any() and (z > 1e38).any()
    want = xyz_np(z, cam).transpose(0, 3, 1, 2)                       # [B,3,h,w]
    dz = _dev(z)
    for fill in (7.0, -3.0):                                           # every output is overwritten by every call
        raw = torch.full((B, 3, h, w), fill, dtype=torch.float32, device="cuda")
        x8 = torch.full((B, h, w, 8), fill, dtype=torch.float32, device="cuda")
        cl = torch.full((B, 3, h, w), fill, dtype=torch.float32, device="cuda")
        _lib.check(lib.quber_op_xyz_from_depth(_p(dz), B, h, w, _cam4(cam), cam.convention_id, flags, _p(raw), _p(x8), _p(cl), _st()))
        got = raw.cpu().numpy()
        assert same_bits(got, np.ascontiguousarray(want)), "raw planes"
        assert np.array_equal(np.isnan(got), np.isnan(want))
        x8p = torch.full_like(x8, 5.0)
        clp = torch.full_like(cl, 5.0)
        _lib.check(lib.quber_op_dsn_pack(_p(raw), B, h, w, flags, _p(x8p), _p(clp), _st()))
        assert torch.equal(x8.view(torch.int32), x8p.view(torch.int32)), "x8 against dsn_pack"
        assert torch.equal(cl.view(torch.int32), clp.view(torch.int32)), "clean against dsn_pack"
        clean = np.where(np.isnan(want), np.float32(0), want)
        if flags & 1:
            clean[:, 1] = -clean[:, 1]
        g = cl.cpu().numpy()
        assert np.array_equal(g.view(np.uint32), clean.view(np.uint32)), "clean against the contract"
        g8 = x8.cpu().numpy()
        assert np.array_equal(g8[..., :3].view(np.uint32), clean.transpose(0, 2, 3, 1).view(np.uint32)) and (g8[..., 3:].view(np.uint32) == 0).all()
    # each output alone
    raw2 = torch.full((B, 3, h, w), 1.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.quber_op_xyz_from_depth(_p(dz), B, h, w, _cam4(cam), cam.convention_id, flags, _p(raw2), None, None, _st()))
    assert torch.equal(raw2.view(torch.int32), raw.view(torch.int32))
    cl2 = torch.full((B, 3, h, w), 1.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.quber_op_xyz_from_depth(_p(dz), B, h, w, _cam4(cam), cam.convention_id, flags, None, None, _p(cl2), _st()))
    assert torch.equal(cl2.view(torch.int32), cl.view(torch.int32))


def test_xyz_from_depth_refusals():
    lib = _lib.load()
    d = torch.zeros((1, 3, 3, 5), dtype=torch.float32, device="cuda")
    cam = _cam4(CAMS["uois"])
    ok = lambda *a: lib.quber_op_xyz_from_depth(*a)
    assert ok(_p(d), 1, 3, 5, cam, 1, 0, _p(d), None, None, _st()) == 0
    assert ok(_p(d), 1, 3, 5, cam, 1, 0, None, None, None, _st()) != 0          # no output
    assert ok(None, 1, 3, 5, cam, 1, 0, _p(d), None, None, _st()) != 0           # no depth
    assert ok(_p(d), 1, 3, 5, None, 1, 0, _p(d), None, None, _st()) != 0         # no camera
    assert ok(_p(d), 1, 3, 5, cam, 2, 0, _p(d), None, None, _st()) != 0          # unknown convention
    assert ok(_p(d), 1, 3, 5, cam, 1, 2, _p(d), None, None, _st()) != 0          # unknown flag bit
    assert ok(_p(d), 0, 3, 5, cam, 1, 0, _p(d), None, None, _st()) != 0
    assert ok(_p(d), 1, 3, 5, (C.c_double * 4)(0.0, 1.0, 0.0, 0.0), 1, 0, _p(d), None, None, _st()) != 0
    assert ok(_p(d), 1, 3, 5, (C.c_double * 4)(1.0, 1.0, float("nan"), 0.0), 1, 0, _p(d), None, None, _st()) != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("convention", ["pinhole", "uois"])
def test_seed_from_depth_equals_seed_from_the_contracts_xyz(convention):
    """DsnEngine.seed(z=, camera=) = seed(xyz=xyz_np(z, camera)), bit for bit, at the smallest feature_dim the plan accepts, B = 1 and 2 of a
    capacity-2 engine; a second call with other data overwrites every output; forward() likewise; the refusals launch nothing."""
    h, w = 48, 80
    cam = CAMS[convention]
    net = DsnEngine(dsn_arch.init_state_dict(3, gain=0.7, feature_dim=8), h, w, max_batch=2)
    assert net.feature_dim == 8
    z = depth_batch(2, h, w, 5)
    z[1] = np.where(np.isfinite(z[1]) & (np.abs(z[1]) < 10), z[1], np.float32(0.9))         # frame 1: ordinary metres throughout
    xyz = np.ascontiguousarray(xyz_np(z, cam).transpose(0, 3, 1, 2))
    for B, order in ((1, [0]), (2, [0, 1]), (2, [1, 0]), (1, [1])):
        dz, dx = _dev(z[order]), _dev(xyz[order])
        a = net.seed(z=dz, camera=cam)
        a = [t.clone() for t in a]
        b = net.seed(dx)
        for got, ref, what in zip(a, b, ("votes", "fg", "classes")):
            assert got.dtype == ref.dtype and got.shape == ref.shape
            if what == "votes":
                assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (what, order)
            else:
                assert torch.equal(got, ref), (what, order)
        la, oa = net.forward(z=dz, camera=cam)
        la, oa = la.clone(), oa.clone()
        lb, ob = net.forward(dx)
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(oa.view(torch.int32), ob.view(torch.int32)), order
    first = net.seed(z=_dev(z[:1]), camera=cam)[2].clone()
    other = net.seed(z=_dev(z[1:]), camera=cam)[2]
    assert not torch.equal(first, other), "the two frames seed alike: the overwrite check shows nothing"
    # the same first op under the profiled entry
    plan = net.profile(z=_dev(z[:1]), camera=cam)
    assert plan[0][0] == "pack" and len(plan) == len(net.profile(_dev(xyz[:1])))
    for bad in (lambda: net.seed(_dev(xyz[:1]), z=_dev(z[:1]), camera=cam), lambda: net.seed(z=_dev(z[:1])), lambda: net.seed(camera=cam),
                lambda: net.seed(z=_dev(z[:1]), camera=(1.0, 1.0, 0.0, 0.0)), lambda: net.seed(z=_dev(z[:1, :, :-1]), camera=cam),
                lambda: net.seed(z=_dev(z[:1].astype(np.float64)), camera=cam), lambda: net.seed(z=torch.from_numpy(z[:1]), camera=cam),
                lambda: net.seed(z=_dev(np.concatenate([z, z])), camera=cam)):
        with pytest.raises(ValueError):
            bad()
    lib = net.eng.lib
    d = _dev(z[:1])
    assert lib.quber_dsn_forward_depth(net.eng.h, _p(d), 1, 0, None, 0, None, None, None, None, None, _st()) != 0
    assert lib.quber_dsn_forward_depth(net.eng.h, None, 1, 0, _cam4(cam), 0, None, None, None, None, None, _st()) != 0
    assert lib.quber_dsn_forward_depth(net.eng.h, _p(d), 1, 0, _cam4(cam), 3, None, None, None, None, None, _st()) != 0
    assert lib.quber_dsn_forward_depth(net.eng.h, _p(d), 3, 0, _cam4(cam), 0, None, None, None, None, None, _st()) != 0
    net.close()


@pytest.mark.parametrize("with_region", [False, True], ids=["cluster", "cluster+region"])
def test_predict_camera_equals_predict_xyz(with_region):
    """MaskRefinerPredictor.predict / predict_batch(depth_z=, camera=) under seeding= [+ region=]: every entry of every dict equals the
    xyz= call's on xyz_np of the same depth; each refusal comes before any launch."""
    from quber_amd import synth
    from quber_amd.gms import IMP, GaussianMeanShift
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
    from quber_amd.region import RegionRefinement
    from test_gpu_cleanup import speck_logits
    from test_gpu_masknms import _equal, _predictor
    f = np.load([p for p in golden("dsn_scene") if "96x128" in p][0])
    h, w = f["xyz"].shape[1:]
    cam = Camera(118.0, 121.0, 63.5, 47.25)
    zs = [np.ascontiguousarray(f["xyz"][2]), np.ascontiguousarray(f["xyz"][2][:, ::-1])]
    assert np.isnan(zs[0]).any()
    xyz = [xyz_np(z, cam) for z in zs]                                  # [h,w,3]
    logits = speck_logits(h, w)
    sc = [synth.make_scene(3 + b, h, w, 2) for b in range(2)]
    rgb, dep = np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])
    gkw = dict(num_seeds=40, sigma=0.3, epsilon=0.3, min_pixels=100, imp=IMP(5, True), seed=5)
    seeding = DepthSeeding(dsn_arch.init_state_dict(int(f["seed"]), gain=float(f["gain"])))
    region = RegionRefinement(rrn_arch.init_state_dict(0, gain=0.7, feature_dim=8), crop=32, chunk=3) if with_region else None
    off1, off2 = [], []
    kw = dict(decode_errors=True, track_initial=True)
    pa = _predictor(h, w, logits, off1, cluster=GaussianMeanShift(**gkw), seeding=seeding, region=region, **kw)
    pb = _predictor(h, w, logits, off2, cluster=GaussianMeanShift(**gkw), seeding=seeding, region=region, **kw)

    def same(a, b, what):
        assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
        assert ("region_ids" in a) == with_region and "seeding_fg" in a and "cluster_ids" in a
        for key in b:
            _equal(a[key], b[key], "%s: %s" % (what, key))

    a = pa.predict(rgb[0], dep[0], depth_z=zs[0], camera=cam)[0]
    b = pb.predict(rgb[0], dep[0], xyz=xyz[0])[0]
    same(a, b, "predict")
    print("clusters", int(a["cluster_report"][0]), "seeding", a["seeding_report"].tolist())
    assert int(a["seeding_report"][2]) > 0, "no foreground: the comparison is of empty frames"
    assert torch.equal(off1[-1], off2[-1])
    outs = pa.predict_batch(rgb, dep, None, depth_z=[zs[1], zs[0]], camera=cam)
    refs = pb.predict_batch(rgb, dep, None, xyz=[xyz[1], xyz[0]])
    for i, (a, b) in enumerate(zip(outs, refs)):
        same(a, b, "predict_batch frame %d" % i)
    # a uois camera through the same path
    cu = Camera(118.0, 121.0, 63.5, 47.25, "uois")
    same(pa.predict(rgb[1], dep[1], depth_z=zs[1], camera=cu)[0], pb.predict(rgb[1], dep[1], xyz=xyz_np(zs[1], cu))[0], "uois")
    n_launched = len(off1)
    plain = MaskRefinerPredictor(None, device="cuda:0", cluster=GaussianMeanShift(**gkw))
    votes = np.zeros((3, h, w), np.float32)
    for call in (lambda: plain.predict(rgb[0], dep[0], depth_z=zs[0], camera=cam),                                  # no seeding=
                 lambda: pa.predict(rgb[0], dep[0], depth_z=zs[0], camera=cam, xyz=xyz[0]),
                 lambda: pa.predict(rgb[0], dep[0], depth_z=zs[0], camera=cam, center_votes=votes),
                 lambda: pa.predict(rgb[0], dep[0], depth_z=zs[0], camera=cam, fg=np.zeros((h, w), np.uint8)),
                 lambda: pa.predict(rgb[0], dep[0], np.zeros((1, h, w), np.uint8), depth_z=zs[0], camera=cam),       # masks
                 lambda: pa.predict_batch(rgb, dep, [np.zeros((1, h, w), np.uint8)] * 2, depth_z=zs, camera=cam),
                 lambda: pa.predict(rgb[0], dep[0], camera=cam),                                                    # no depth_z=
                 lambda: pa.predict(rgb[0], dep[0], depth_z=zs[0][:, :-1], camera=cam),                             # shape
                 lambda: pa.predict(rgb[0], dep[0], depth_z=zs[0].astype(np.float64), camera=cam),                  # dtype
                 lambda: pa.predict(rgb[0], dep[0], depth_z=(zs[0] * 1000).astype(np.uint16), camera=cam),
                 lambda: pa.predict_batch(rgb, dep, None, depth_z=zs[:1], camera=cam),                              # one plane for two frames
                 lambda: pa.predict(rgb[0], dep[0], depth_z=zs[0], camera=(118.0, 121.0, 63.5, 47.25)),
                 lambda: pa.model.enqueue_batch(_dev(rgb), _dev(dep), _dev(np.zeros((2, 1, h, w), np.uint8)), camera=cam)):
        with pytest.raises(ValueError):
            call()
    assert len(off1) == n_launched
    seeding.close()
    if region is not None:
        region.close()
    for p in (pa, pb, plain):
        p.model.close()
