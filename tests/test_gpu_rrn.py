"""GPU: the Region Refinement Network of UOIS-Net-3D (csrc/rrn.hip, csrc/plan_rrn.hip, quber_amd/region) against the fixtures generated from
the imported reference module, against the staged restatement tests/rrn_torch.py and against the numpy contract of tests/test_rrn_cpu.py,
for both heads (option key 54: convolution + 1x1 head / the collapsed 3x3 filter).

Layer by layer (test_rrn_layers): one forward at batch 3 of a capacity-4 engine, then every launch is held to the staged restatement
evaluated in float64 ON THE DEVICE'S OWN INPUTS of that launch, with the bars of tests/test_gpu_dsn.py (u = 2^-24):
  pack, max pool         exact
  dense convolutions     max |err| / max(1, max |ref|) < 2e-6
  GroupNorm, bilinear    |err| <= 2e-6 + 1e-5 |ref|
  head, key 0            (fd + 1) u sum |w| |f|: a chain of fd fused multiply-adds
  head, key 1            (9 fd + 2) u sum |w'| |x| with the float64 w': a chain of 9 fd fused multiply-adds, and the one rounding
                         of w' (u |w'| |x| per term)
The gather / scatter (test_rrn_hooks) equals the numpy contract bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rrn_torch as R
from conftest import golden
from quber_amd import _lib, engine as qengine, rrn_arch
from quber_amd.region import RegionRefinement, RrnEngine, standardize_table
from test_rrn_cpu import contract_cases, load_scene, rrn_crop_np, rrn_paste_np, standardize_table_np
from test_zoom_cpu import zoom_rois_np

pytestmark = pytest.mark.gpu
TOL = 1e-4
U = 2.0 ** -24


def _w(sd, dtype, device="cpu"):
    return {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in sd.items()}


def _within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                        # a NaN is outside every bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst {ratio:.2f}x, max error {float(err.max()):.3e}"
    return ratio


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("head", [0, 1], ids=["conv+1x1", "collapsed"])
@pytest.mark.parametrize("path", golden("rrn_net"), ids=os.path.basename)
def test_rrn_golden(path, head):
    z = np.load(path)
    S = z["rgb"].shape[-1]
    sd = rrn_arch.init_state_dict(int(z["seed"]), gain=float(z["gain"]), feature_dim=int(z["feature_dim"]))
    net = RrnEngine(sd, S, 3, head=head)
    assert net.eng.get_option(54) == head and net.feature_dim == 64
    rgb, mask = torch.from_numpy(z["rgb"]), torch.from_numpy(z["mask"])
    o = net.run(rgb.cuda(), mask.cuda())
    lg, ref = o["logits"].cpu(), o["refined"].cpu()
    err = float(np.abs(lg.numpy() - z["logits"]).max())
    print(f"{os.path.basename(path)} head {head}: max |HIP - reference f32| {err:.3e} (ref_f32_err {float(z['ref_f32_err']):.3e})")
    assert err < TOL
    with torch.no_grad():
        r64 = R.forward(rgb.double(), mask, _w(sd, torch.float64))
    hip = (lg.double() - r64).abs().reshape(2, -1).max(1).values.numpy()
    o32 = (torch.from_numpy(z["logits"]).double() - r64).abs().reshape(2, -1).max(1).values.numpy()
    for i in range(2):
        print(f"PARITY-E2E | {os.path.basename(path)} head {head} crop {i} | HIP {hip[i]:.3e} | torch-fp32 {o32[i]:.3e} | ratio {hip[i] / o32[i]:.2f}")
    assert (hip <= 2 * o32).all(), (hip, o32)
    agree = float((ref.numpy() == (z["logits"] > 0)).mean())
    print(f"mask agreement {agree:.6f} (near_zero_share {float(z['near_zero_share']):.2e})")
    assert agree > 0.999
    assert ref.dtype == torch.uint8 and torch.equal(ref, (lg > 0).to(torch.uint8))
    assert torch.equal(net.forward(rgb.cuda(), mask.cuda()).cpu(), lg)
    # another threshold, other inputs: every output is overwritten
    o2 = net.run(rgb.flip(0).contiguous().cuda(), mask.flip(0).contiguous().cuda(), threshold=0.7, out=o)
    assert o2["logits"] is o["logits"]
    assert torch.equal(o2["logits"].cpu(), lg.flip(0)) and torch.equal(o2["refined"].cpu(), (lg.flip(0) > float(np.float32(np.log(0.7 / 0.3)))).to(torch.uint8))
    # the refusals launch nothing
    lib = net.eng.lib
    p = lambda t: C.c_void_p(t.data_ptr())
    d = rgb.cuda()
    assert lib.quber_forward(net.eng.h, p(d), p(d), p(d), 1, p(d), None) != 0 and b"quber_rrn_forward" in lib.quber_last_error()
    assert lib.quber_dsn_forward(net.eng.h, p(d), 1, 0, p(d), None, None, None, None, None) != 0
    assert lib.quber_rrn_forward(net.eng.h, p(d), p(mask.cuda()), 2, C.c_float(0.0), None, None, None) != 0
    assert lib.quber_rrn_forward(net.eng.h, p(d), p(mask.cuda()), 4, C.c_float(0.0), p(o["logits"]), None, None) != 0
    plain = qengine.Engine(qengine.make_config(S, S, with_network=False))
    assert lib.quber_rrn_forward(plain.h, p(d), p(mask.cuda()), 1, C.c_float(0.0), p(o["logits"]), None, None) != 0
    plain.close()
    with pytest.raises(ValueError):
        RrnEngine(sd, 40, 1)
    net.close()


class _Forward:
    """one forward with every tap read back as float64 NCHW"""

    def __init__(self, S, fd, head, n, cap):
        self.sd = rrn_arch.init_state_dict(seed=3, feature_dim=fd)
        rgb, mask = R.synth_crops(n, S, 44)
        mask[1] = 0                                                   # one crop with an empty mask, one with a full one
        mask[2] = 7
        self.rgb, self.mask = torch.from_numpy(rgb), torch.from_numpy(mask)
        net = RrnEngine(self.sd, S, cap, head=head)
        self.logits = net.run(self.rgb.cuda(), self.mask.cuda(), refined=False)["logits"].cpu()
        self.plan = net.eng.plan()
        names = {s.out for s in R.plan(head) if s.out not in R.OUTPUTS} | set(R.CONCAT)
        self.taps = {k: net.eng.debug_tensor(k, n).cpu() for k in sorted(names)}
        net.close()

    def get(self, name):
        if name == "rgb":
            return self.rgb.double()
        if name == "mask":
            return self.mask
        if name == "logits":
            return self.logits.double()
        return self.taps[name].double().permute(0, 3, 1, 2)


_HEADS = ("conv+1x1", "collapsed")
LAYER_CASES = [(fd, head) for fd in (8, 12, 20, 44, 60) for head in (0, 1)]
LAYER_IDS = [_HEADS[head] if fd == 8 else f"fd{fd}-{_HEADS[head]}" for fd, head in LAYER_CASES]


@pytest.mark.parametrize("feature_dim,head", LAYER_CASES, ids=LAYER_IDS)
def test_rrn_layers(feature_dim, head):
    """S = 32: the maps are 32, 16, 8, 4 and 2 pixels wide; batch 3 of a capacity-4 engine.  feature_dim 8, and widths that route the
    convolutions otherwise: 12 and 44 (channel counts that are no multiple of 8), 20 (whole K slices of 32 from 160 channels on), 60
    (the last staged chunk of rr_head3_kernel is 12 channels)."""
    S, fd = 32, feature_dim
    fw = _Forward(S, fd, head, 3, 4)
    assert int(fw.sd["encoder.layer1.layer1.conv1.weight"].shape[0]) == fd
    w64 = _w(fw.sd, torch.float64)
    failures, kinds = [], {}
    for st in R.plan(head):
        ins = [i.take(fw.get) for i in st.ins]
        got = fw.get(st.out)
        with torch.no_grad():
            ref = st.fn(w64, *ins)
        assert got.shape == ref.shape, st.out
        e_hip = float((got.double() - ref.double()).abs().max())
        note = ""
        try:
            if st.kind in ("pack8", "pool"):
                assert torch.equal(got, ref), st.out
                note = "exact"
            elif st.kind == "conv":
                rel = e_hip / max(1.0, float(ref.abs().max()))
                note = f"rel {rel:.2e} of 2e-6"
                assert rel < 2e-6, f"{st.out}: {rel:.3e}"
            elif st.kind in ("gn", "bilinear"):
                note = f"{_within(got, ref, 2e-6 + 1e-5 * ref.abs(), st.out):.2f} of the bound"
            elif st.kind == "head":
                wk = w64["fg_module.weight"]
                note = f"{_within(got, ref, (fd + 1) * U * F.conv2d(ins[0].abs(), wk.abs())[:, 0], st.out):.2f} of the bound"
            else:
                assert st.kind == "head3"
                w9, b = R.collapsed(w64)
                note = f"{_within(got, ref, (9 * fd + 2) * U * F.conv2d(ins[0].abs(), w9.abs(), None, 1, 1)[:, 0], st.out):.2f} of the bound"
        except AssertionError as ex:
            failures.append(str(ex))
            note += " FAILED"
        kinds[st.kind] = kinds.get(st.kind, 0) + 1
        print(f"PARITY-OP | S {S} fd {fd} head {head} | {st.op} | {st.out} | {st.kind} | HIP {e_hip:.3e} | {note}")
    assert not failures, "\n".join(failures)
    assert [n for n, _, _, _ in fw.plan] == R.ops(head)
    assert kinds["gn"] == 19 and kinds["pool"] == 4 and kinds["bilinear"] == 4 and kinds["conv"] == (19 if head else 20)
    for name, parts in R.CONCAT.items():
        assert torch.equal(fw.get(name), torch.cat([fw.get(p) for p in parts], 1)), name
    x = fw.get("X")
    assert x.shape[1] == 8 and not x[:, 4:].any() and set(np.unique(x[:, 3].numpy())) == {0.0, 1.0} and x[2, 3].all() and not x[1, 3].any()
    with torch.no_grad():
        r32 = R.forward(fw.rgb, fw.mask, _w(fw.sd, torch.float32))
        r64 = R.forward(fw.rgb.double(), fw.mask, w64)
    hip = (fw.logits.double() - r64).abs().reshape(3, -1).max(1).values.numpy()
    o32 = (r32.double() - r64).abs().reshape(3, -1).max(1).values.numpy()
    print(f"PARITY-E2E | batch 3 of 4, S {S} fd {fd} head {head} | HIP {hip} | torch-fp32 {o32}")
    assert float((fw.logits - r32).abs().max()) < TOL and (hip <= 2 * o32).all()


@pytest.fixture(scope="module")
def ref224():
    """the restatement at the workload's own size, once for both heads: float32 on the device, float64 on the host (a few seconds)"""
    sd = rrn_arch.init_state_dict(0, gain=0.7, feature_dim=64)
    rgb, mask = (torch.from_numpy(t) for t in R.synth_crops(2, 224, 71))
    with torch.no_grad():
        r64 = R.forward(rgb.double(), mask, _w(sd, torch.float64)).cuda()
        rgb, mask = rgb.cuda(), mask.cuda()
        r32 = R.forward(rgb, mask, _w(sd, torch.float32, "cuda"))
    return sd, rgb, mask, r32, r64


@pytest.mark.parametrize("head", [0, 1], ids=["conv+1x1", "collapsed"])
def test_rrn_224(ref224, head):
    """S = 224, feature_dim 64, batch 2: the 14 x 14 and 28 x 28 maps take convolution routes that no small test takes."""
    sd, rgb, mask, r32, r64 = ref224
    net = RrnEngine(sd, 224, 2, head=head)
    lg = net.forward(rgb, mask)
    err = float((lg - r32).abs().max())
    hip = (lg.double() - r64).abs().reshape(2, -1).max(1).values.cpu().numpy()
    o32 = (r32.double() - r64).abs().reshape(2, -1).max(1).values.cpu().numpy()
    for i in range(2):
        print(f"PARITY-E2E | S 224 head {head} crop {i} | HIP {hip[i]:.3e} | torch-fp32 {o32[i]:.3e} | ratio {hip[i] / o32[i]:.2f} | max |HIP - torch-fp32| {err:.3e}")
    net.close()
    assert err < TOL
    assert (hip <= 2 * o32).all(), (hip, o32)


def _p(t, elems=0):
    return C.c_void_p(t.data_ptr() + 4 * elems if t is not None else 0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("S,fd", [(16, 8), (48, 8), (16, 24), (16, 64), (48, 64), (16, 12), (16, 44), (48, 60)], ids=lambda v: str(v))
def test_rrn_head_hooks(S, fd):
    """rrn_head3 and rrn_head on a channel slice of a wider buffer holding 1e3 elsewhere, batch 2 of 3, the input shifted by 40: a kernel that pads
    with anything but zero, reads the next frame's rows or a foreign channel misses the bound by orders of magnitude.  48 is three tiles of 16; 24 channels are a staged chunk of 16 and one of 8;
    12, 44 and 60 channels end in a staged chunk of 12: three quads, so the staging loop's split of its index into (pixel, quad) is a division by 3;
    the frames behind the batch and the other outputs stay untouched."""
    lib = _lib.load()
    rng = np.random.default_rng(S * 100 + fd)
    B, cap, cs, c0 = 2, 3, fd + 12, 4
    buf = np.full((cap, S, S, cs), 1e3, np.float32)
    data = (rng.standard_normal((cap, S, S, fd)) + 40.0).astype(np.float32)
    buf[..., c0:c0 + fd] = data
    x = torch.from_numpy(data).double().permute(0, 3, 1, 2)[:B]
    w9 = (rng.standard_normal((fd, 3, 3)) / np.sqrt(9 * fd)).astype(np.float32)
    bias, thr = np.float32(0.3), np.float32(0.1)
    w9t = torch.from_numpy(w9).double()[None]
    ref = F.conv2d(x, w9t, torch.tensor([float(bias)], dtype=torch.float64), 1, 1)[:, 0]
    bound = (9 * fd + 2) * U * F.conv2d(x.abs(), w9t.abs(), None, 1, 1)[:, 0]
    xd, wd = _dev(buf), _dev(w9.reshape(fd, 9).T)                      # [9][fd], tap-major
    for _ in range(2):                                                 # the second call overwrites the first
        lg = torch.full((cap, S, S), 5.0, dtype=torch.float32, device="cuda")
        rf = torch.full((cap, S, S), 9, dtype=torch.uint8, device="cuda")
        _lib.check(lib.quber_op_rrn_head3(_p(xd, c0), cs, B, S, S, fd, _p(wd), C.c_float(bias), C.c_float(thr), _p(lg), rf.data_ptr(), _st()))
    lgh, rfh = lg.cpu(), rf.cpu()
    ratio = _within(lgh[:B].double(), ref, bound, f"rrn_head3 S {S} fd {fd}")
    print(f"PARITY-HOOK | rrn_head3 | S {S} fd {fd} | max error {float((lgh[:B].double() - ref).abs().max()):.3e} | {ratio:.3f} of the bound | max |ref| {float(ref.abs().max()):.1f}")
    assert (lgh[B:] == 5.0).all() and (rfh[B:] == 9).all() and torch.equal(rfh[:B], (lgh[:B] > float(thr)).to(torch.uint8))
    lg2 = torch.full((cap, S, S), 5.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.quber_op_rrn_head3(_p(xd, c0), cs, B, S, S, fd, _p(wd), C.c_float(bias), C.c_float(thr), _p(lg2), None, _st()))
    rf2 = torch.full((cap, S, S), 9, dtype=torch.uint8, device="cuda")
    _lib.check(lib.quber_op_rrn_head3(_p(xd, c0), cs, B, S, S, fd, _p(wd), C.c_float(bias), C.c_float(thr), None, rf2.data_ptr(), _st()))
    assert torch.equal(lg2.cpu(), lgh) and torch.equal(rf2.cpu(), rfh)
    # the 1x1 head
    w1 = (rng.standard_normal(fd) / np.sqrt(fd)).astype(np.float32)
    w1t = torch.from_numpy(w1).double()[None, :, None, None]
    lg3 = torch.full((cap, S, S), 5.0, dtype=torch.float32, device="cuda")
    rf3 = torch.full((cap, S, S), 9, dtype=torch.uint8, device="cuda")
    w1d = _dev(w1)
    _lib.check(lib.quber_op_rrn_head(_p(xd, c0), cs, B, S, S, fd, _p(w1d), C.c_float(thr), _p(lg3), rf3.data_ptr(), _st()))
    l3 = lg3.cpu()
    ratio = _within(l3[:B].double(), F.conv2d(x, w1t)[:, 0], (fd + 1) * U * F.conv2d(x.abs(), w1t.abs())[:, 0], f"rrn_head S {S} fd {fd}")
    print(f"PARITY-HOOK | rrn_head | S {S} fd {fd} | {ratio:.3f} of the bound")
    assert (l3[B:] == 5.0).all() and torch.equal(rf3.cpu()[:B], (l3[:B] > float(thr)).to(torch.uint8)) and (rf3.cpu()[B:] == 9).all()
    # refused views launch nothing
    assert lib.quber_op_rrn_head3(_p(xd, c0), fd - 4, B, S, S, fd, _p(wd), C.c_float(0), C.c_float(0), _p(lg), None, _st()) != 0
    assert lib.quber_op_rrn_head3(_p(xd, c0), cs, B, S, S, fd, _p(wd), C.c_float(0), C.c_float(0), None, None, _st()) != 0
    assert lib.quber_op_rrn_head(_p(xd, c0 + 1), cs, B, S, S, fd, _p(wd), C.c_float(0), _p(lg), None, _st()) != 0
    torch.cuda.synchronize()


def test_rrn_pack_hook():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    B, h, w = 2, 5, 11
    rgb = rng.standard_normal((3, 3, h, w)).astype(np.float32)
    rgb[0, 1, 2, 3] = -0.0
    mask = rng.integers(0, 3, (3, h, w)).astype(np.uint8) * 100
    x8 = torch.full((3, h, w, 8), 9.0, dtype=torch.float32, device="cuda")
    d_rgb, d_mask = _dev(rgb), _dev(mask)                              # (named: a temporary's memory may be handed out again before the launch)
    _lib.check(lib.quber_op_rrn_pack(_p(d_rgb), d_mask.data_ptr(), B, h, w, _p(x8), _st()))
    got = x8.cpu().numpy()
    assert np.array_equal(got[:B, ..., :3].view(np.uint32), rgb[:B].transpose(0, 2, 3, 1).view(np.uint32))
    assert np.array_equal(got[:B, ..., 3], (mask[:B] != 0).astype(np.float32)) and (got[:B, ..., 4:].view(np.uint32) == 0).all() and (got[B:] == 9.0).all()
    assert lib.quber_op_rrn_pack(_p(d_rgb), None, B, h, w, _p(x8), _st()) != 0


def _crop_paste(img, ids, n_ids, rois, slots, z, refined, S, n_masks, cap=None):
    """Engine.rrn_crop / rrn_paste of a network-less engine of capacity `cap` against the contract, bit for bit"""
    B, h, w = ids.shape
    eng = qengine.Engine(qengine.make_config(h, w, max_batch=cap or B, with_network=False))
    d_ids, d_slots = _dev(ids.astype(np.int32)), _dev(np.asarray(slots, np.int32).reshape(-1, 2))
    d_rois = eng.zoom_rois(d_ids, n_ids, 0.25)
    assert np.array_equal(d_rois.cpu().numpy(), rois)
    tab = standardize_table()
    assert np.array_equal(tab.view(np.uint32), standardize_table_np().view(np.uint32))
    T = len(slots)
    want_rgb, want_mask = rrn_crop_np(img, ids, slots, rois, tab, S)
    if T:
        out = (torch.full((T, 3, S, S), 7.0, dtype=torch.float32, device="cuda"), torch.full((T, S, S), 7, dtype=torch.uint8, device="cuda"))
        rgb, mask = eng.rrn_crop(_dev(img), d_ids, d_slots, d_rois, _dev(tab), S, out=out)
        assert np.array_equal(rgb.cpu().numpy().view(np.uint32), want_rgb.view(np.uint32)), "rgb crops"
        assert np.array_equal(mask.cpu().numpy(), want_mask), "mask crops"
    want = rrn_paste_np(refined, slots, rois, z, B, h, w, n_masks)
    o = None
    for fill in (77, 3):                                               # every output is overwritten by every call
        o = {"ids": torch.full((B, h, w), fill, dtype=torch.int32, device="cuda"), "masks": torch.full((B, n_masks, h, w), fill, dtype=torch.uint8, device="cuda"),
             "source": torch.full((B, n_masks), fill, dtype=torch.int32, device="cuda"), "keys": torch.full((T,), float(fill), dtype=torch.float32, device="cuda"),
             "report": torch.full((B, 4), fill, dtype=torch.int32, device="cuda")}
        eng.rrn_paste(_dev(refined), d_slots, d_rois, _dev(z), B, n_masks, out=o)
        for k in ("ids", "masks", "source", "report"):
            assert np.array_equal(o[k].cpu().numpy(), want[k]), k
        assert np.array_equal(o["keys"].cpu().numpy().view(np.uint32), want["keys"].view(np.uint32)), "keys"
    eng.close()
    return want


@pytest.mark.parametrize("path", golden("rrn_scene"), ids=os.path.basename)
def test_rrn_crop_paste_scenes(path):
    z, img, ids, n_ids, slots, zz, S = load_scene(path)
    rois = zoom_rois_np(ids, n_ids, 0.25)
    want = _crop_paste(img, ids, n_ids, rois, slots, zz, z["refined"], S, n_ids)
    lut = np.concatenate([[0], want["source"][0]])
    assert np.array_equal(lut[want["ids"][0]], z["painted"])          # and with that the device equals the reference's painted map


def test_rrn_crop_paste_cases():
    """an empty refined crop, a full crop, a 1 x 1 ROI, equal keys, slots out of range, an absent id; two frames of a capacity-3 engine; fewer
    planes than ids; no slots at all"""
    img, ids, n_ids, rois, slots, z, refined, S = contract_cases()
    _crop_paste(img, ids, n_ids, rois, slots, z, refined, S, n_ids, cap=3)
    _crop_paste(img, ids, n_ids, rois, slots, z, refined, S, 2, cap=3)
    _crop_paste(img, ids, n_ids, rois, slots[:0], z, refined[:0], S, 3)
    eng = qengine.Engine(qengine.make_config(40, 56, max_batch=1, with_network=False))
    d = _dev(np.zeros((1, 40, 56), np.int32))
    p = lambda t: C.c_void_p(t.data_ptr())
    assert eng.lib.quber_rrn_paste(eng.h, None, None, None, p(d), 2, 0, 0, S, 1, p(d), p(d), p(d), None, p(d), None) != 0        # batch above the capacity
    assert eng.lib.quber_rrn_paste(eng.h, None, None, None, p(d), 1, 0, 0, S, 0, p(d), p(d), p(d), None, p(d), None) != 0        # no planes
    assert eng.lib.quber_rrn_crop(eng.h, p(d), p(d), p(d), p(d), p(d), 1, 300, 1, S, p(d), p(d), None) != 0
    eng.close()


# ---- the predictor ----
REGION_KEYS = {"region_masks", "region_ids", "region_source", "region_rois", "region_report"}


def test_predict_region():
    """96 x 128 frames through seeding= + cluster=GaussianMeanShift() + region=RegionRefinement(crop=32): region_* equal the numpy contract
    applied to the call's own cluster_ids and the network engine's own refined crops; the refiner's encoded initial masks are the refined ones
    (the stub forward of tests/test_gpu_masknms.py records them); region=None gives the parent's dicts; the refusals come before any launch."""
    from quber_amd import dsn_arch, synth
    from quber_amd.gms import IMP, GaussianMeanShift
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
    from quber_amd.meanshift import MeanShift
    from quber_amd.seeding import DepthSeeding
    from test_gpu_cleanup import speck_logits
    from test_gpu_masknms import _equal, _predictor
    z = np.load([p for p in golden("dsn_scene") if "96x128" in p][0])
    h, w = z["xyz"].shape[1:]
    S = 32
    logits = speck_logits(h, w)
    sc = [synth.make_scene(3 + b, h, w, 2) for b in range(2)]
    rgb, dep = np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])
    xyz = [z["xyz"], np.ascontiguousarray(z["xyz"][:, :, ::-1])]
    gkw = dict(num_seeds=40, sigma=0.3, epsilon=0.3, min_pixels=100, imp=IMP(5, True), seed=5)
    seeding = DepthSeeding(dsn_arch.init_state_dict(int(z["seed"]), gain=float(z["gain"])))
    rsd = rrn_arch.init_state_dict(0, gain=0.7, feature_dim=8)
    region = RegionRefinement({"model": {"module." + k: torch.from_numpy(v) for k, v in rsd.items()}}, crop=S, chunk=3)
    kw = dict(decode_errors=True, track_initial=True)
    off1, off2 = [], []
    refined = _predictor(h, w, logits, off1, cluster=GaussianMeanShift(**gkw), seeding=seeding, region=region, **kw)
    plain = _predictor(h, w, logits, off2, cluster=GaussianMeanShift(**gkw), seeding=seeding, **kw)
    assert plain.region is None

    def check(a, b, frame, what):
        assert set(a) - REGION_KEYS == set(b) and REGION_KEYS <= set(a) and not REGION_KEYS & set(b), (what, sorted(a), sorted(b))
        for key in [k for k in b if k.startswith(("cluster_", "seeding_"))]:
            _equal(a[key], b[key], "%s: %s" % (what, key))                # the stages before the network are untouched
        ids = a["cluster_ids"].cpu().numpy()[None]
        n = int(a["cluster_report"][0])
        assert n >= 2, "fewer than two clusters: the comparison would be empty"
        n_ids = a["cluster_masks"].shape[0]
        rois = zoom_rois_np(ids, n_ids, 0.25)
        assert np.array_equal(a["region_rois"].cpu().numpy(), rois[0, :n])
        slots = np.array([(0, j) for j in range(1, n + 1)], np.int32)
        crop_rgb, crop_mask = rrn_crop_np(rgb[frame][None], ids, slots, rois, standardize_table_np(), S)
        net = region.engine_for(refined.device)
        ref = torch.cat([net.run(_dev(crop_rgb[i:i + 3]), _dev(crop_mask[i:i + 3]), logits=False)["refined"] for i in range(0, n, 3)]).cpu().numpy()
        zz = np.ascontiguousarray(xyz[frame][2])[None]
        want = rrn_paste_np(ref, slots, rois, zz, 1, h, w, n_ids)
        k = int(want["report"][0, 0])
        assert a["region_report"].dtype == torch.int64 and a["region_report"].tolist() == want["report"][0].tolist(), what
        assert np.array_equal(a["region_ids"].cpu().numpy(), want["ids"][0]) and a["region_ids"].dtype == torch.int32, what
        assert np.array_equal(a["region_masks"].cpu().numpy(), want["masks"][0, :k]) and a["region_masks"].dtype == torch.uint8, what
        assert a["region_source"].dtype == torch.int64 and a["region_source"].tolist() == want["source"][0, :k].tolist(), what
        assert k >= 1 and not np.array_equal(want["ids"][0], ids[0]), "the network changed nothing: the comparison shows nothing"
        return want["masks"][0]

    a = refined.predict(rgb[0], dep[0], xyz=xyz[0])[0]
    b = plain.predict(rgb[0], dep[0], xyz=xyz[0])[0]
    m0 = check(a, b, 0, "predict")
    # the pass's initial masks are the refined ones: what the refiner encoded equals the encoding of the refined masks
    eng = refined.model.engine_for(h, w, 1, m0.shape[0])
    assert torch.equal(off1[-1], eng.encode(_dev(m0[None])))
    assert not torch.equal(off1[-1], off2[-1])
    # depth_z= beside center_votes= / fg=: a fresh clustering stream, so its first draw is that of the call above
    v, f, _ = seeding.engine_for(h, w, 1, refined.device).seed(_dev(xyz[0][None]))
    votes = _predictor(h, w, logits, [], cluster=GaussianMeanShift(**gkw), region=region, **kw)
    c = votes.predict(rgb[0], dep[0], center_votes=v[0].cpu().numpy(), fg=f[0].cpu().numpy(), depth_z=np.nan_to_num(xyz[0][2]))[0]
    for key in REGION_KEYS:
        _equal(c[key], a[key], "depth_z: " + key)
    outs = refined.predict_batch(rgb, dep, None, xyz=[xyz[1], xyz[0]])
    refs = plain.predict_batch(rgb, dep, None, xyz=[xyz[1], xyz[0]])
    xyz = [xyz[1], xyz[0]]
    for i, (a, b) in enumerate(zip(outs, refs)):
        check(a, b, i, "predict_batch frame %d" % i)
    # the refusals; none of them launches anything
    n_launched = len(off1)
    for call in (lambda: votes.predict(rgb[0], dep[0], center_votes=v[0].cpu().numpy(), fg=f[0].cpu().numpy()),                  # no z plane
                 lambda: votes.predict(rgb[0], dep[0], center_votes=v[0].cpu().numpy(), fg=f[0].cpu().numpy(), depth_z=np.zeros((h, w + 1), np.float32)),
                 lambda: refined.predict(rgb[0], dep[0], xyz=xyz[0], depth_z=xyz[0][2]),
                 lambda: refined.predict(rgb[0], dep[0], np.zeros((1, h, w), np.uint8)),                                        # masks
                 lambda: refined.model.enqueue_batch(_dev(rgb), _dev(dep), _dev(np.zeros((2, 1, h, w), np.uint8))),
                 lambda: MaskRefinerPredictor(None, device="cuda:0", region=region),                                           # no cluster=
                 lambda: MaskRefinerPredictor(None, device="cuda:0", region=region, cluster=MeanShift(num_seeds=8)),
                 lambda: MaskRefinerPredictor(None, device="cuda:0", region="rrn", cluster=GaussianMeanShift(**gkw)),
                 lambda: RegionRefinement(rsd, crop=40),
                 lambda: RegionRefinement(rsd, threshold=1.0)):
        with pytest.raises(ValueError):
            call()
    assert len(off1) == n_launched
    region.close()
    seeding.close()
    for p in (refined, plain, votes):
        p.model.close()
