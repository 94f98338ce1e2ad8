"""GPU: LMFFNet foreground network + 30 % overlap post-filter against the fixtures generated
from the imported reference module and against the oracle restatement.

Layer by layer (test_lmffnet_layers): one forward at batch 3 of a capacity-4 engine, then every launch of the plan is held to
the staged oracle (oracle.lmffnet_torch.plan) evaluated in float64 ON THE DEVICE'S OWN INPUTS of that launch, so an error
cannot hide behind the layers after it and the failing launch is named.  Bars, from the arithmetic (u = 2^-24):
  dense convolutions       max |err| / max(1, max |ref|) < 2e-6, the bar of test_conv_igemm_vs_torch for the exact-fp32 kernels
  depthwise 3x3            12 u (|scale| sum |x w| + |shift|) per element: nine fused multiply-adds and the affine one
  BN + PReLU of a [sum]    3 u (|a| + |b|) |scale| + u |shift|: the addition and the fused multiply-add
  max pool                 exact;   average pool  10 u sum |x| / 9: eight additions and the division
  channel scale            2 ulp of the result: one multiplication
  bilinear x2, upsample    5 u sum w |x| over the four neighbours: at the factors 2 and 4 the source coordinates and the weights w are
                           exact, and every path to the result is product, sum, product, sum - four roundings
  PMCA weights, MAD gate   expf has no published bound: HIP's max error <= 2 x that of float32 torch on the same input + 1 ulp of
                           the output (two correct fp32 evaluations differ by summation order; the factor covers that only)
The depthwise and BN + PReLU kernels take the FOLDED float32 scale / shift vectors the plan uploads (csrc/plan_lmff.hip bnp());
their bound is the kernel's, so the float64 reference is evaluated on those vectors, restated here operation by operation.  A
PReLU multiplies an error by at most max(1, |slope|).  A second assert holds the result to the unfolded float64 parameters with
the fold's own four roundings added (4 u on the scale, 5 u |mean scale| + u |shift| on the shift)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import lmffnet_torch as L
from quber_amd import lmff_arch, synth
from quber_amd.foreground.predictor import LmffEngine, filter_masks, lmffNet

pytestmark = pytest.mark.gpu
TOL = 1e-4
U = 2.0 ** -24


def _w(sd, dtype):
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


def _oracle_errors(lg_hip, x, sd):
    """(max |HIP - f64|, max |oracle f32 - f64|) per frame of x"""
    with torch.no_grad():
        r32 = L.forward(x, _w(sd, torch.float32)).double()
        r64 = L.forward(x.double(), _w(sd, torch.float64))
    B = x.shape[0]
    hip = (torch.from_numpy(lg_hip).double() - r64).abs().reshape(B, -1).max(1).values
    o32 = (r32 - r64).abs().reshape(B, -1).max(1).values
    return hip.numpy(), o32.numpy(), r32.float().numpy()


@pytest.mark.parametrize("path", golden("lmffnet"), ids=os.path.basename)
def test_lmffnet_golden(path):
    z = np.load(path)
    h, w = z["rgb"].shape[:2]
    sd = lmff_arch.init_state_dict(seed=int(z["seed"]))
    net = LmffEngine(sd, h, w, 2)
    rgb2, dep2 = np.stack([z["rgb"], z["rgb"][::-1].copy()]), np.stack([z["depth"], z["depth"][::-1].copy()])
    bgr = torch.from_numpy(rgb2).cuda()
    dep = torch.from_numpy(dep2).cuda()
    lg = net.logits(bgr, dep).cpu().numpy()
    assert np.abs(lg[0] - z["logits"]).max() < TOL
    # both frames against the oracle: HIP is no further from the float64 evaluation than twice the fp32 oracle's own distance
    x = torch.cat([L.preprocess(rgb2[i], dep2[i]) for i in range(2)])
    hip, o32, r32 = _oracle_errors(lg, x, sd)
    assert np.abs(lg[1] - r32[1]).max() < TOL          # the flipped frame
    for i in range(2):
        print(f"PARITY-E2E | {os.path.basename(path)} frame {i} | HIP {hip[i]:.3e} | torch-fp32 {o32[i]:.3e} | ratio {hip[i] / o32[i]:.2f}")
    assert (hip <= 2 * o32).all(), (hip, o32)
    fg, _ = net.foreground(bgr, dep)
    agree = (fg[0].cpu().numpy().astype(bool) == L.foreground_mask(z["logits"])).mean()
    assert agree > 0.999
    net.eng.close()


# ---- layer by layer ----
def _fold(sd, bn):
    """csrc/plan_lmff.hip bnp() in float32, operation by operation: (scale, shift) of BN(eps 1e-3)"""
    g, b, m, v = (sd[f"{bn}.bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g * (np.float32(1.0) / np.sqrt(v + np.float32(1e-3)))
    shift = b - m * scale
    assert scale.dtype == np.float32 and shift.dtype == np.float32
    return scale, shift


def _folded(w64, sd, bn):
    """the weight dict with BN `bn` replaced by one that applies the folded float32 vectors: y = x * scale + shift"""
    scale, shift = _fold(sd, bn)
    w = dict(w64)
    w[bn + ".bn.weight"], w[bn + ".bn.bias"] = torch.from_numpy(scale).double(), torch.from_numpy(shift).double()
    w[bn + ".bn.running_mean"] = torch.zeros(len(scale), dtype=torch.float64)
    w[bn + ".bn.running_var"] = torch.full((len(scale),), 1.0 - 1e-3, dtype=torch.float64)
    return w


def _bn_terms(w64, sd, bn):
    """per-channel [1,C,1,1] float64: folded |scale|, |shift|, PReLU gain max(1, |slope|), and the fold's own error as
    (relative on the scale, absolute on the shift)"""
    scale, shift = _fold(sd, bn)
    e = lambda a: torch.as_tensor(a, dtype=torch.float64).abs()[None, :, None, None]
    s64 = w64[bn + ".bn.weight"] / torch.sqrt(w64[bn + ".bn.running_var"] + 1e-3)
    fold_shift = 5 * U * (w64[bn + ".bn.running_mean"] * s64).abs() + U * e(shift)[0, :, 0, 0]
    return e(scale), e(shift), e(w64[bn + ".acti.weight"]).clamp(min=1.0), 4 * U, e(fold_shift)


def _within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                        # a NaN is outside every bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst {ratio:.2f}x, max error {float(err.max()):.3e}"
    return ratio


class _Forward:
    """one forward at batch 3 of a capacity-4 engine with every tap read back as float64 NCHW"""

    def __init__(self, h, w):
        self.sd = lmff_arch.init_state_dict(seed=3)
        scenes = [synth.make_scene(s, h, w, 3) for s in (21, 22, 23)]
        rgb = np.stack([s["rgb"] for s in scenes])
        dep = np.stack([s["depth"] for s in scenes])
        dep[1] = 0                                                   # one frame without depth: exact zeros through the injections
        self.rgb, self.dep = rgb, dep
        net = LmffEngine(self.sd, h, w, 4)
        self.logits = net.logits(torch.from_numpy(rgb).cuda(), torch.from_numpy(dep).cuda()).cpu().double()
        self.num_ops = net.eng.lib.quber_num_ops(net.eng.h)
        self.plan = net.eng.plan()                                   # [(name, kind, flops, launches)] in execution order
        self.h4, self.w4 = h // 4, w // 4
        names = {"X", "A", "Bc", "Cc"} | {s.out for s in L.plan() if s.out != "logits"} | set(L.ALIAS)
        names |= {n + ".buf" for n in ("FFM_A.bn_prelu", "FFM_A.conv1x1", "FFM_B1.bn_prelu", "FFM_B1.conv1x1", "FFM_B2.bn_prelu",
                                       "FFM_B2.conv1x1", "MAD.DwConv2", "MAD.PwConv1", "MAD.PwConv2", "MAD.up_out", "inject_2.0",
                                       "inject_3.0", "inject_3.1")}
        self.taps = {n: net.eng.debug_tensor(n, 3).cpu() for n in sorted(names)}
        net.eng.close()

    def get(self, name):
        if name == "logits":
            return self.logits
        t = self.taps[name].double()                                 # [3,H,W,C]
        if name.endswith(".weights"):
            return t.reshape(3, -1)
        if name == "MAD.gate":
            return t.reshape(3, 3, self.h4, self.w4)
        return t.permute(0, 3, 1, 2)


_FORWARDS = {}


def _forward(h, w):
    if (h, w) not in _FORWARDS:
        _FORWARDS[(h, w)] = _Forward(h, w)
    return _FORWARDS[(h, w)]


@pytest.mark.parametrize("size", [(72, 88), (64, 96)], ids=["72x88", "64x96"])
def test_lmffnet_layers(size):
    """Every launch of the plan against the staged float64 oracle on the launch's own device inputs, three different frames at batch 3
    of a capacity-4 engine.  72 x 88: the stride-8 map is 9 x 11, odd both ways; 64 x 96: it is 8 x 12, smaller than the dilations 16
    and 32, so only the centre tap of those layers meets the map."""
    fw = _forward(*size)
    sd = fw.sd
    w64, w32 = _w(sd, torch.float64), _w(sd, torch.float32)
    steps = L.plan()
    checked, failures = [], []
    for st in steps:
        ins = [i.take(fw.get) for i in st.ins]
        got = fw.get(st.out)
        with torch.no_grad():
            ref = st.fn(w64, *ins)
            t32 = st.fn(w32, *[i.float() for i in ins]).double()
        assert got.shape == ref.shape, st.out
        e_hip, e_t32 = float((got - ref).abs().max()), float((t32 - ref).abs().max())
        note = ""
        try:
            if st.kind == "conv":
                rel = e_hip / max(1.0, float(ref.abs().max()))
                note = f"rel {rel:.2e} of 2e-6"
                assert rel < 2e-6, f"{st.out}: {rel:.3e}"
            elif st.kind in ("dwconv", "affine"):
                with torch.no_grad():
                    ref_f = st.fn(_folded(w64, sd, st.bn), *ins)
                scale, shift, gain, fold_scale, fold_shift = _bn_terms(w64, sd, st.bn)
                if st.kind == "dwconv":
                    x = ins[0]
                    mag = F.conv2d(x.abs(), w64[st.key + ".conv.weight"].abs(), None, 1, st.dil, st.dil, x.shape[1])
                    bound = 12 * U * (scale * mag + shift)
                else:
                    mag = sum(i.abs() for i in ins)
                    bound = 3 * U * mag * scale + U * shift
                ratio = _within(got, ref_f, gain * bound, st.out)
                _within(got, ref, gain * (bound + fold_scale * scale * mag + fold_shift), st.out + " (unfolded parameters)")
                e_hip = float((got - ref_f).abs().max())
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "maxpool":
                assert torch.equal(got, ref), st.out
                note = "exact"
            elif st.kind == "avgpool":
                ratio = _within(got, ref, 10 * U * F.avg_pool2d(ins[0].abs(), 3, 2, 1), st.out)
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "scale":
                ratio = _within(got, ref, 2 * torch.from_numpy(np.spacing(ref.abs().float().numpy())).double(), st.out)
                note = f"{ratio:.2f} of the bound"
            elif st.kind in ("bilinear", "upsample"):
                mag = F.interpolate(ins[0].abs(), ref.shape[-2:], mode="bilinear", align_corners=False)
                ratio = _within(got, ref, 5 * U * mag, st.out)
                note = f"{ratio:.2f} of the bound"
            else:
                assert st.kind in ("pmca", "gate")
                ulp = float(np.spacing(np.float32(ref.abs().max())))
                note = f"allowed {2 * e_t32 + ulp:.3e}"
                assert e_hip <= 2 * e_t32 + ulp, f"{st.out}: HIP {e_hip:.3e}, float32 torch {e_t32:.3e}, 1 ulp {ulp:.3e}"
        except AssertionError as ex:
            failures.append(str(ex))
            note += " FAILED"
        print(f"PARITY-OP | {size[0]}x{size[1]} | {st.op} | {st.out} | {st.kind} | HIP {e_hip:.3e} | torch-fp32 {e_t32:.3e} | {note}")
        checked.append((st.op, st.out, st.kind))
    assert not failures, "\n".join(failures)
    # every op of the plan was held to its reference exactly once, in the plan's own order and under the plan's own name: the plan
    # names an op after the tap it writes (a convolution after its weight key, the two two-launch ops after their last / first tap)
    assert fw.num_ops == 96 == len(fw.plan)
    by_op = [[(out, kind) for op, out, kind in checked if op == i] for i in range(fw.num_ops)]
    assert [op for op, _, _ in checked] == sorted(op for op, _, _ in checked) and sum(len(b) for b in by_op) == len(checked) == 99
    for i, ((name, kind, _, _), mine) in enumerate(zip(fw.plan, by_op)):
        assert [k for _, k in mine] in (["pmca", "scale"], ["gate", "upsample"]) or len(mine) == 1, (i, name, mine)
        assert name in [out for out, _ in mine] and (kind == "conv") == (mine[0][1] == "conv"), (i, name, kind, mine)


@pytest.mark.parametrize("size", [(72, 88), (64, 96)], ids=["72x88", "64x96"])
def test_lmffnet_buffers_and_pad_channels(size):
    """The preprocessed input is the oracle's to the bit; the concatenation buffers hold their producers' outputs side by side; the
    pad channels of every wide buffer a narrower slice is written into are still exactly zero after the forward (no launch writes
    outside its slice); the four short tap names are the long ones."""
    fw = _forward(*size)
    x = torch.cat([L.preprocess(fw.rgb[i], fw.dep[i]) for i in range(3)]).double()
    X = fw.get("X")
    assert X.shape[1] == 8 and torch.equal(X[:, :6], x)
    for name, parts in L.CONCAT.items():
        buf = fw.get(name)
        cat = torch.cat([fw.get(p) for p in parts], 1)
        assert torch.equal(buf[:, :cat.shape[1]], cat), name
    pads = {"X": 6, "A": 38, "FFM_A.bn_prelu.buf": 38, "FFM_A.conv1x1.buf": 38, "Bc": 134, "FFM_B1.bn_prelu.buf": 134,
            "FFM_B1.conv1x1.buf": 134, "Cc": 262, "FFM_B2.bn_prelu.buf": 262, "FFM_B2.conv1x1.buf": 262, "MAD.DwConv2.buf": 262,
            "MAD.PwConv1.buf": 3, "MAD.PwConv2.buf": 3, "MAD.up_out.buf": 3, "inject_2.0.buf": 6, "inject_3.0.buf": 6,
            "inject_3.1.buf": 6}
    for name, c in pads.items():
        buf = fw.taps[name]                                          # float32 NHWC as read
        assert buf.shape[3] in (c + 1, c + 2) and buf.shape[3] % 4 == 0, name
        assert (buf[..., c:].numpy().view(np.uint32) == 0).all(), f"{name}: pad channels {c}.. were written"
        assert float(buf[..., :c].abs().max()) > 0, name
    for short, long in L.ALIAS.items():
        assert torch.equal(fw.taps[short], fw.taps[long]), short


def test_lmffnet_batch_below_capacity_end_to_end():
    """All three frames of the batch-3 forwards (capacity 4) against the oracle: the parent's 1e-4 on the fp32 oracle, and HIP no further
    from the float64 evaluation than twice the fp32 oracle's own distance."""
    for size in ((72, 88), (64, 96)):
        fw = _forward(*size)
        x = torch.cat([L.preprocess(fw.rgb[i], fw.dep[i]) for i in range(3)])
        lg = fw.logits.float().numpy()
        hip, o32, r32 = _oracle_errors(lg, x, fw.sd)
        assert np.abs(lg - r32).max() < TOL
        for i in range(3):
            print(f"PARITY-E2E | batch 3 of 4, {size[0]}x{size[1]} frame {i} | HIP {hip[i]:.3e} | torch-fp32 {o32[i]:.3e} | ratio {hip[i] / o32[i]:.2f}")
        assert (hip <= 2 * o32).all(), (hip, o32)


def test_lmffnet_full_frame_and_filter():
    sd = lmff_arch.init_state_dict(seed=3)
    sc = synth.make_scene(4, 480, 640, 10)
    w = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        ref = L.forward(L.preprocess(sc["rgb"], sc["depth"]), w)[0].numpy()
    net = LmffEngine(sd, 480, 640, 1)
    bgr, dep = torch.from_numpy(sc["rgb"][None]).cuda(), torch.from_numpy(sc["depth"][None]).cuda()
    masks = (sc["masks"] != 0)
    lg = net.logits(bgr, dep).cpu().numpy()[0]
    assert np.abs(lg - ref).max() < TOL
    fg, counts = net.foreground(bgr, dep, torch.from_numpy(masks.astype(np.uint8)[None]).cuda())
    fg_np = fg[0].cpu().numpy().astype(bool)
    # integer counts are exact for the HIP foreground mask; the kept set equals the reference rule on that mask
    c = counts[0].cpu().numpy()
    for k, m in enumerate(masks):
        assert c[k, 0] == np.sum(m & fg_np) and c[k, 1] == np.sum(m)
    kept = filter_masks(list(masks), counts[0])
    exp = L.overlap_filter(list(masks), fg_np)
    assert len(kept) == len(exp) and all(np.array_equal(a, b) for a, b in zip(kept, exp))
    net.eng.close()


def test_lmffnet_predictor_dropin(tmp_path):
    from PIL import Image
    sc = synth.make_scene(6, 480, 640, 4)
    Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / "rgb.png")
    Image.fromarray((sc["depth"][:, :, 0].astype(np.uint16) * 5 + 300)).save(tmp_path / "depth.png")
    with pytest.warns(UserWarning):
        p = lmffNet(str(tmp_path / "missing.pth"))
    fg = p.predict(str(tmp_path / "rgb.png"), str(tmp_path / "depth.png"))
    assert fg.shape == (480, 640) and fg.dtype == np.bool_
    from quber_amd.eval.refiner_model import MaskRefiner
    ref = MaskRefiner(None, None, dataset="OSD", foreground_filter=True, lmffnet_weights=str(tmp_path / "missing.pth"))
    masks, out, secs, fgm = ref.predict(str(tmp_path / "rgb.png"), str(tmp_path / "depth.png"), sc["masks"] != 0, None)
    assert fgm is not None and fgm.shape == (480, 640)
