"""GPU: CGNet, the foreground network of the UOAIS base model, and the filter built on it (csrc/cgnet.hip, csrc/plan_cgnet.hip,
quber_amd/foreground/predictor.py) against the fixtures generated from the imported reference module and against the staged
restatement tests/cgnet_torch.py, for both plans (option key 52: fused blocks / separate launchers).

Layer by layer (test_cgnet_layers): one forward at batch 3 of a capacity-4 engine, then every launch is held to the staged restatement
evaluated in float64 ON THE DEVICE'S OWN INPUTS of that launch.  Bars, from the arithmetic (u = 2^-24):
  dense convolutions    max |err| / max(1, max |ref|) < 2e-6, the bar of the exact-fp32 convolution kernels (tests/test_gpu_lmffnet.py)
  depthwise 3x3         12 u (|scale| sum |x w| + |shift|): nine fused multiply-adds and the affine one, on the folded float32 vectors
  BN + PReLU            3 u |a| |scale| + u |shift|;  average pool  10 u sum |x| / 9
  fused joint kernel    per output channel, with t the float64 1x1 + BN + PReLU of the launch's input and E1 = 2e-6 max(1, max |t|) the
                        dense bar on it:  12 u (|scale2| sum |t w| + |shift2|)  +  |scale2| (sum |w| over the taps inside the map) E1
                        - the depthwise bound evaluated on the exact t, plus what an error of E1 on every t does to the sum
  a PReLU multiplies an error by at most max(1, |slope|): every bound above is multiplied by that gain of the launch's last PReLU
  means                 2 u |mean|: the tile sums and their total are float64, only the quotient is rounded to float32
  the FC gate           expf has no published bound: HIP's max error <= 2 x that of float32 torch on the same input + 1 ulp of the output
  scale [+ residual]    u (|x| + 2 |joi y|) + 2^-150: one product (which may underflow) and one sum;   x8 upsample  5 u sum w |x| over the four neighbours
The stand-alone hooks (test_cgnet_hooks) hold the two kernels of a block to the same bars on the smallest shapes that still go
wrong, including a BN shift large against the data: a kernel that zero-pads x instead of t puts prelu(shift) into the halo and
misses the joint bound at the border by orders of magnitude."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cgnet_torch as G
from conftest import golden
from quber_amd import _lib, cgnet_arch, synth
from quber_amd.foreground.predictor import CGNet, CgnetEngine, filter_masks_uoais

pytestmark = pytest.mark.gpu
TOL = 1e-4
U = 2.0 ** -24


def _w(sd, dtype):
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


def _oracle_errors(lg_hip, x, sd):
    """(max |HIP - f64|, max |restatement f32 - f64|) per frame of x, and the float32 restatement"""
    with torch.no_grad():
        r32 = G.forward(x, _w(sd, torch.float32)).double()
        r64 = G.forward(x.double(), _w(sd, torch.float64))
    B = x.shape[0]
    hip = (torch.from_numpy(lg_hip).double() - r64).abs().reshape(B, -1).max(1).values
    o32 = (r32 - r64).abs().reshape(B, -1).max(1).values
    return hip.numpy(), o32.numpy(), r32.float().numpy()


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("path", golden("cgnet_scene"), ids=os.path.basename)
def test_cgnet_golden(path, fused):
    z = np.load(path)
    h, w = z["rgb"].shape[:2]
    sd = cgnet_arch.init_state_dict(int(z["seed"]), gain=float(z["gain"]))
    net = CgnetEngine(sd, h, w, 3, fused=fused)
    assert net.eng.get_option(52) == fused
    rgb2, dep2 = np.stack([z["rgb"], z["rgb"][::-1].copy()]), np.stack([z["depth"], z["depth"][::-1].copy()])
    bgr, dep = torch.from_numpy(rgb2).cuda(), torch.from_numpy(dep2).cuda()
    lg = net.logits(bgr, dep).cpu().numpy()
    err = float(np.abs(lg[0] - z["logits"]).max())
    print(f"{os.path.basename(path)} fused {fused}: max |HIP - reference f32| {err:.3e} (ref_f32_err {float(z['ref_f32_err']):.3e})")
    assert err < TOL
    x = torch.cat([G.preprocess(rgb2[i], dep2[i]) for i in range(2)])
    hip, o32, r32 = _oracle_errors(lg, x, sd)
    for i in range(2):
        print(f"PARITY-E2E | {os.path.basename(path)} fused {fused} frame {i} | HIP {hip[i]:.3e} | torch-fp32 {o32[i]:.3e} | ratio {hip[i] / o32[i]:.2f}")
    assert np.abs(lg[1] - r32[1]).max() < TOL          # the flipped frame
    assert (hip <= 2 * o32).all(), (hip, o32)
    fg, _ = net.foreground(bgr, dep)
    agree = (fg[0].cpu().numpy() == G.foreground_mask(z["logits"])).mean()
    print(f"foreground agreement {agree:.6f} (near_tie_share {float(z['near_tie_share']):.2e})")
    assert agree > 0.999
    net.eng.close()


# ---- the float64 references of the kernels that take folded vectors ----
def _fold(sd, bn):
    """csrc/plan_cgnet.hip bnp() in float32, operation by operation: (scale, shift) of the BN(eps 1e-3) under `bn`.*"""
    g, b, m, v = (sd[f"{bn}.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
    scale = g * (np.float32(1.0) / np.sqrt(v + np.float32(1e-3)))
    shift = b - m * scale
    assert scale.dtype == np.float32 and shift.dtype == np.float32
    return scale, shift


def _col(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)[None, :, None, None]


def _affine_prelu(t, scale, shift, slope):
    v = t * _col(scale) + _col(shift)
    return torch.where(v > 0, v, v * _col(slope))


def _dw(t, w9, dil):
    return F.conv2d(t, w9, None, 1, dil, dil, t.shape[1])


def _dw_bound(t, w9, dil, scale, shift, slope, e_in=0.0):
    """gain x (12 u (|scale| sum |t w| + |shift|) + |scale| (sum |w| inside the map) e_in)"""
    mag = _dw(t.abs(), w9.abs(), dil)
    wsum = _dw(torch.ones_like(t), w9.abs(), dil)
    gain = _col(slope).abs().clamp(min=1.0)
    return gain * (12 * U * (_col(scale).abs() * mag + _col(shift).abs()) + _col(scale).abs() * wsum * e_in)


def _joint_ref_and_bound(x, w1, bn1, wloc, wsur, bn2, dil):
    """x float64 [B,C,h,w]; w1 [C/2,C]; bn1 = (scale, shift, slope) of the 1x1 (float32 vectors, applied as the kernel does); wloc / wsur
    [C/2,1,3,3]; bn2 the concatenation's.  -> (float64 joi, bound): the composition spelled out in the module docstring."""
    ch = w1.shape[0]
    t = _affine_prelu(F.conv2d(x, w1[:, :, None, None]), *bn1)
    e1 = 2e-6 * max(1.0, float(t.abs().max()))
    ref, bound = [], []
    for wk, d, lo in ((wloc, 1, 0), (wsur, dil, ch)):
        s, h, a = (v[lo:lo + ch] for v in bn2)
        ref.append(_affine_prelu(_dw(t, wk, d), s, h, a))
        bound.append(_dw_bound(t, wk, d, s, h, a, e1))
    return torch.cat(ref, 1), torch.cat(bound, 1)


def _within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                        # a NaN is outside every bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst {ratio:.2f}x, max error {float(err.max()):.3e}"
    return ratio


def _gate_check(got, m, gate_fn, what):
    """HIP's error <= 2 x float32 torch's on the same input + 1 ulp"""
    with torch.no_grad():
        ref, t32 = gate_fn(m, torch.float64), gate_fn(m, torch.float32).double()
    e_hip, e_t32 = float((got - ref).abs().max()), float((t32 - ref).abs().max())
    ulp = float(np.spacing(np.float32(ref.abs().max())))
    assert e_hip <= 2 * e_t32 + ulp, f"{what}: HIP {e_hip:.3e}, float32 torch {e_t32:.3e}, 1 ulp {ulp:.3e}"
    return e_hip, e_t32, ulp


def _apply_bound(joi, y, x):
    jy = (joi * y[:, :, None, None]).abs()
    # (a saturated gate makes joi y subnormal: there the product's rounding error is absolute, at most half the smallest subnormal)
    return U * ((0 if x is None else x.abs()) + 2 * jy) * (1 + 1e-6) + 2.0 ** -150


# ---- layer by layer ----
class _Forward:
    """one forward at batch 3 of a capacity-4 engine with every tap read back as float64 NCHW"""

    def __init__(self, h, w, fused):
        self.sd = cgnet_arch.init_state_dict(seed=3)
        scenes = [synth.make_scene(s, h, w, 3) for s in (21, 22, 23)]
        rgb = np.stack([s["rgb"] for s in scenes])
        dep = np.stack([s["depth"] for s in scenes])
        dep[1] = 0                                                   # one frame without depth
        self.rgb, self.dep = rgb, dep
        net = CgnetEngine(self.sd, h, w, 4, fused=fused)
        self.logits = net.logits(torch.from_numpy(rgb).cuda(), torch.from_numpy(dep).cuda()).cpu().double()
        self.plan = net.eng.plan()
        names = {"X", "A", "Bc", "Cc", "b1.buf", "bn_prelu_2.buf", "classifier.0.buf", "inject_2.0.buf"} | {s.out for s in G.plan(fused) if s.out != "logits"}
        self.taps = {n: net.eng.debug_tensor(n, 3).cpu() for n in sorted(names)}
        net.eng.close()

    def get(self, name):
        if name == "logits":
            return self.logits
        t = self.taps[name].double()                                 # [3,H,W,C]
        if name.endswith(".F_glo.mean") or name.endswith(".F_glo.y"):
            return t.reshape(3, -1)
        return t.permute(0, 3, 1, 2)


_FORWARDS = {}


def _forward(h, w, fused):
    if (h, w, fused) not in _FORWARDS:
        _FORWARDS[(h, w, fused)] = _Forward(h, w, fused)
    return _FORWARDS[(h, w, fused)]


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
def test_cgnet_layers(fused):
    """56 x 72: the stage maps are 14 x 18 and 7 x 9 - neither a multiple of the 8 x 8 tile, the 7-row map smaller than the dilated
    reach of 9 rows, so whole filter rows of the dilated depthwise convolution lie in the padding."""
    h, w = 56, 72
    fw = _forward(h, w, fused)
    sd = fw.sd
    w64, w32 = _w(sd, torch.float64), _w(sd, torch.float32)
    steps = G.plan(bool(fused))
    failures, kinds = [], {}
    for st in steps:
        ins = [i.take(fw.get) for i in st.ins]
        got = fw.get(st.out)
        with torch.no_grad():
            ref = st.fn(w64, *ins)
        assert got.shape == ref.shape, st.out
        note = ""
        e_hip = float((got - ref).abs().max())
        try:
            if st.kind == "conv":
                rel = e_hip / max(1.0, float(ref.abs().max()))
                note = f"rel {rel:.2e} of 2e-6"
                assert rel < 2e-6, f"{st.out}: {rel:.3e}"
            elif st.kind == "dwconv":
                c = ins[0].shape[1]
                scale, shift = (v[st.lo:st.lo + c] for v in _fold(sd, st.act + ".bn"))
                slope = sd[st.act + ".act.weight"][st.lo:st.lo + c]
                w9 = w64[st.key + ".conv.weight"]
                ref_f = _affine_prelu(_dw(ins[0], w9, st.dil), scale, shift, slope)
                ratio = _within(got, ref_f, _dw_bound(ins[0], w9, st.dil, scale, shift, slope), st.out)
                # the unfolded float64 parameters: the fold's own four roundings added (4 u on the scale, 5 u |mean scale| + u |shift| on the shift)
                s64 = (w64[st.act + ".bn.weight"] / torch.sqrt(w64[st.act + ".bn.running_var"] + 1e-3))[st.lo:st.lo + c]
                fold = 4 * U * _col(s64).abs() * _dw(ins[0].abs(), w9.abs(), st.dil) + 5 * U * _col(w64[st.act + ".bn.running_mean"][st.lo:st.lo + c] * s64).abs() + U * _col(shift).abs()
                _within(got, ref, _dw_bound(ins[0], w9, st.dil, scale, shift, slope) + _col(slope).abs().clamp(min=1.0) * fold, st.out + " (unfolded parameters)")
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "affine":
                scale, shift = _fold(sd, st.act + ".bn")
                slope = sd[st.act + ".act.weight"]
                ref_f = _affine_prelu(ins[0], scale, shift, slope)
                gain = _col(slope).abs().clamp(min=1.0)
                ratio = _within(got, ref_f, gain * (3 * U * ins[0].abs() * _col(scale).abs() + U * _col(shift).abs()), st.out)
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "avgpool":
                ratio = _within(got, ref, 10 * U * F.avg_pool2d(ins[0].abs(), 3, 2, 1), st.out)
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "joint":
                n = st.key
                ch = ins[0].shape[1] // 2
                bn1 = _fold(sd, n + ".conv1x1.bn") + (sd[n + ".conv1x1.act.weight"],)
                bn2 = _fold(sd, n + ".bn_prelu.bn") + (sd[n + ".bn_prelu.act.weight"],)
                ref_f, bound = _joint_ref_and_bound(ins[0], w64[n + ".conv1x1.conv.weight"].reshape(ch, 2 * ch), bn1, w64[n + ".F_loc.conv.weight"],
                                                    w64[n + ".F_sur.conv.weight"], bn2, st.dil)
                ratio = _within(got, ref_f, bound, st.out)
                # and against the unfolded float64 parameters: both folds' roundings are inside E1 and the 12 u, up to the factor 2
                _within(got, ref, 2 * bound, st.out + " (unfolded parameters)")
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "concat":
                assert torch.equal(got, ref), st.out
                note = "exact"
            elif st.kind == "mean":
                ratio = _within(got, ref, 2 * U * ref.abs(), st.out)
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "gate":
                e_hip, e_t32, ulp = _gate_check(got, ins[0], lambda m, dt: st.fn(w64 if dt == torch.float64 else w32, m.to(dt)), st.out)
                note = f"allowed {2 * e_t32 + ulp:.3e}"
            elif st.kind == "apply":
                ratio = _within(got, ref, _apply_bound(ins[0], ins[1], ins[2] if len(ins) > 2 else None), st.out)
                note = f"{ratio:.2f} of the bound"
            else:
                assert st.kind == "upsample"
                mag = F.interpolate(ins[0].abs(), ref.shape[-2:], mode="bilinear", align_corners=False)
                ratio = _within(got, ref, 5 * U * mag, st.out)
                note = f"{ratio:.2f} of the bound"
        except AssertionError as ex:
            failures.append(str(ex))
            note += " FAILED"
        kinds[st.kind] = kinds.get(st.kind, 0) + 1
        print(f"PARITY-OP | {h}x{w} fused {fused} | {st.op} | {st.out} | {st.kind} | HIP {e_hip:.3e} | {note}")
    assert not failures, "\n".join(failures)
    # the plan's ops are the restatement's, in order and under the same names; every op but the sums launches was held to a reference
    assert [n for n, _, _, _ in fw.plan] == G.ops(bool(fused))
    assert len(fw.plan) == (67 if fused else 133)
    assert kinds.get("joint", 0) == (22 if fused else 0) and kinds["apply"] == 24 and kinds["mean"] == 24 and kinds["gate"] == 24
    # the preprocessed input is the restatement's to the bit; the pad channels of every wide buffer are still exactly zero
    x = torch.cat([G.preprocess(fw.rgb[i], fw.dep[i]) for i in range(3)]).double()
    X = fw.get("X")
    assert X.shape[1] == 8 and torch.equal(X[:, :4], x)
    for name, parts in G.CONCAT.items():
        cat = torch.cat([fw.get(p) for p in parts], 1)
        assert torch.equal(fw.get(name)[:, :cat.shape[1]], cat), name
    for name, c in {"X": 4, "A": 36, "b1.buf": 36, "Bc": 132, "bn_prelu_2.buf": 132, "classifier.0.buf": 2, "inject_2.0.buf": 4}.items():
        buf = fw.taps[name]
        assert buf.shape[3] % 4 == 0 and buf.shape[3] > c, name
        assert (buf[..., c:].numpy().view(np.uint32) == 0).all(), f"{name}: pad channels {c}.. were written"
        assert float(buf[..., :c].abs().max()) > 0, name
    # end to end, all three frames
    hip, o32, r32 = _oracle_errors(fw.logits.float().numpy(), x.float(), sd)
    assert np.abs(fw.logits.float().numpy() - r32).max() < TOL
    for i in range(3):
        print(f"PARITY-E2E | batch 3 of 4, {h}x{w} fused {fused} frame {i} | HIP {hip[i]:.3e} | torch-fp32 {o32[i]:.3e} | ratio {hip[i] / o32[i]:.2f}")
    assert (hip <= 2 * o32).all(), (hip, o32)


# ---- the stand-alone hooks ----
def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


class _Block:
    """random parameters of one context-guided block on the device, and the two kernels run through the hooks"""

    def __init__(self, c, dil, seed, big_shift):
        rng = np.random.default_rng(seed)
        ch, r = c // 2, 8
        f = lambda *s, sd=1.0: (rng.standard_normal(s) * sd).astype(np.float32)
        self.c, self.ch, self.r, self.dil = c, ch, r, dil
        self.w1 = f(ch, c, sd=np.sqrt(2.0 / c))
        self.bn1 = (rng.uniform(0.6, 1.4, ch).astype(np.float32), (f(ch, sd=0.1) + (40.0 if big_shift else 0.0)).astype(np.float32),
                    rng.uniform(0.1, 0.4, ch).astype(np.float32))
        self.wloc, self.wsur = f(ch, 1, 3, 3, sd=0.4), f(ch, 1, 3, 3, sd=0.4)
        self.bn2 = (rng.uniform(0.6, 1.4, c).astype(np.float32), f(c, sd=0.1), rng.uniform(0.1, 0.4, c).astype(np.float32))
        self.fc0, self.b0, self.fc2, self.b2 = f(r, c, sd=np.sqrt(1.0 / c)), f(r, sd=0.2), f(c, r, sd=np.sqrt(1.0 / r)), f(c, sd=0.2)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.dev = {k: d(v) for k, v in dict(w1=self.w1, s1=self.bn1[0], h1=self.bn1[1], a1=self.bn1[2], wloc=self.wloc, wsur=self.wsur, s2=self.bn2[0],
                                             h2=self.bn2[1], a2=self.bn2[2], fc0=self.fc0, b0=self.b0, fc2=self.fc2, b2=self.b2).items()}
        self.lib = _lib.load()

    def joint(self, xbuf, c0, B, h, w, joi, partials, tiles):
        """xbuf [B,h,w,cs] device NHWC, the input view starts at channel c0"""
        d, st = self.dev, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return self.lib.quber_op_cgnet_joint(C.c_void_p(xbuf.data_ptr() + 4 * c0), xbuf.shape[3], _p(joi), joi.shape[3], B, h, w, self.c, self.dil, _p(d["w1"]),
                                             _p(d["s1"]), _p(d["h1"]), _p(d["a1"]), _p(d["wloc"]), _p(d["wsur"]), _p(d["s2"]), _p(d["h2"]), _p(d["a2"]),
                                             _p(partials), tiles, st)

    def apply(self, joi, xbuf, c0, obuf, o0, B, h, w, partials, tiles, mean, y):
        d, st = self.dev, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        xp = C.c_void_p(xbuf.data_ptr() + 4 * c0) if xbuf is not None else C.c_void_p(0)
        return self.lib.quber_op_cgnet_apply(_p(joi), joi.shape[3], xp, xbuf.shape[3] if xbuf is not None else 0, C.c_void_p(obuf.data_ptr() + 4 * o0),
                                             obuf.shape[3], B, h, w, self.c, self.r, _p(partials), tiles, _p(d["fc0"]), _p(d["b0"]), _p(d["fc2"]), _p(d["b2"]),
                                             _p(mean), _p(y), st)

    def gate(self, m, dtype):
        t = lambda a: torch.from_numpy(a).to(dtype)
        hid = F.relu(F.linear(m.to(dtype), t(self.fc0), t(self.b0)))
        return torch.sigmoid(F.linear(hid, t(self.fc2), t(self.b2)))


HOOK_SHAPES = [(7, 9, 128, 4), (14, 18, 64, 2), (30, 40, 128, 4), (1, 1, 64, 2), (5, 33, 64, 2)]


@pytest.mark.parametrize("big_shift", [False, True], ids=["", "big-shift"])
@pytest.mark.parametrize("shape", HOOK_SHAPES, ids=lambda s: "%dx%dx%d-d%d" % s)
def test_cgnet_hooks(shape, big_shift):
    h, w, c, dil = shape
    B, pad = 3, 8
    blk = _Block(c, dil, 100 + h, big_shift)
    lib = blk.lib
    rng = np.random.default_rng(7 + w)
    cs = c + 2 * pad                                     # every view is a channel slice of a wider buffer: cs > C
    frames = rng.standard_normal((5, h, w, cs)).astype(np.float32)
    tiles = lib.quber_op_cgnet_tiles(h, w, 1)
    assert tiles == -(-h // 8) * -(-w // 8) and lib.quber_op_cgnet_tiles(h, w, 0) == -(-h * w // 64)

    def run(idx, residual):
        xbuf = torch.from_numpy(frames[idx]).cuda()
        joi = torch.full((B, h, w, cs), 7.0, device="cuda")          # the joint kernel writes channels 0 .. C of a wider pixel
        obuf = torch.full((B, h, w, cs), 9.0, device="cuda")
        partials = torch.full((B, tiles, c), float("nan"), dtype=torch.float64, device="cuda")
        mean, y = torch.empty((B, c), device="cuda"), torch.empty((B, c), device="cuda")
        _lib.check(blk.joint(xbuf, pad, B, h, w, joi, partials, tiles))
        _lib.check(blk.apply(joi, xbuf if residual else None, pad, obuf, pad, B, h, w, partials, tiles, mean, y))
        torch.cuda.synchronize()
        return joi.cpu(), obuf.cpu(), mean.cpu(), y.cpu(), partials.cpu()

    joi, out, mean, y, partials = run([0, 1, 2], True)
    x64 = torch.from_numpy(frames[[0, 1, 2]][..., pad:pad + c]).double().permute(0, 3, 1, 2)
    t64 = lambda a: torch.from_numpy(a).double()
    ref, bound = _joint_ref_and_bound(x64, t64(blk.w1), blk.bn1, t64(blk.wloc), t64(blk.wsur), blk.bn2, dil)
    got = joi[..., :c].double().permute(0, 3, 1, 2)
    ratio = _within(got, ref, bound, "joint")
    print(f"PARITY-HOOK | {shape} big_shift {big_shift} | joint {ratio:.2f} of the bound, max |ref| {float(ref.abs().max()):.2f}")
    if big_shift:      # what padding x instead of t would have cost at the border: orders of magnitude above the bound there
        wrong = _affine_prelu(torch.zeros(1, c // 2, 1, 1, dtype=torch.float64), *blk.bn1).abs().min()
        assert float(wrong) > 1e3 * float(bound.max())
    assert (joi[..., c:] == 7.0).all(), "joint wrote outside its channel slice"
    # the tile sums are exact float64 sums of what was written; the mean is their rounded quotient
    assert torch.isfinite(partials).all()
    m_ref = got.mean((2, 3))
    _within(mean.double(), m_ref, 2 * U * m_ref.abs(), "mean")
    _gate_check(y.double(), mean.double(), blk.gate, "gate")
    o_got = out[..., pad:pad + c].double().permute(0, 3, 1, 2)
    _within(o_got, G.apply(got, y.double(), x64), _apply_bound(got, y.double(), x64), "apply + residual")
    assert (out[..., :pad] == 9.0).all() and (out[..., pad + c:] == 9.0).all(), "apply wrote outside its channel slice"
    # no residual; and the sums kernel's partials give the same mean to the bound
    joi2, out2, mean2, y2, _ = run([0, 1, 2], False)
    assert torch.equal(joi2, joi) and torch.equal(mean2, mean) and torch.equal(y2, y), "two runs differ"
    _within(out2[..., pad:pad + c].double().permute(0, 3, 1, 2), G.apply(got, y.double()), _apply_bound(got, y.double(), None), "apply")
    stiles = lib.quber_op_cgnet_tiles(h, w, 0)
    sp = torch.full((B, stiles, c), float("nan"), dtype=torch.float64, device="cuda")
    jd = joi.cuda()
    mean3 = torch.empty((B, c), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.quber_op_cgnet_sums(_p(jd), cs, B, h, w, c, _p(sp), stiles, st))
    ob = torch.empty((B, h, w, c), device="cuda")
    _lib.check(blk.apply(jd, None, 0, ob, 0, B, h, w, sp, stiles, mean3, None))
    torch.cuda.synchronize()
    _within(mean3.cpu().double(), m_ref, 2 * U * m_ref.abs(), "mean over the sums kernel's partials")
    # a frame's result does not depend on its batch neighbours, bit for bit
    joi4, out4, mean4, y4, _ = run([3, 0, 4], True)
    assert torch.equal(joi4[1], joi[0]) and torch.equal(out4[1], out[0]) and torch.equal(mean4[1], mean[0]) and torch.equal(y4[1], y[0])


def test_cgnet_hooks_refuse_bad_views():
    """a refused view returns an error and launches nothing: the output keeps its fill"""
    blk = _Block(64, 2, 1, False)
    lib, B, h, w = blk.lib, 1, 4, 4
    x = torch.zeros((B, h, w, 72), device="cuda")
    joi = torch.full((B, h, w, 64), 3.0, device="cuda")
    tiles = lib.quber_op_cgnet_tiles(h, w, 1)
    partials = torch.zeros((B, tiles, 64), dtype=torch.float64, device="cuda")
    x70 = torch.zeros((B, h, w, 70), device="cuda")
    assert blk.joint(x70, 0, B, h, w, joi, partials, tiles) != 0 and b"groups of 4" in lib.quber_last_error()       # cs % 4
    assert blk.joint(x, 1, B, h, w, joi, partials, tiles) != 0                                                       # misaligned first channel
    assert blk.joint(x, 0, B, h, w, joi, partials, tiles + 1) != 0 and b"tile count" in lib.quber_last_error()
    blk.dil = 5
    assert blk.joint(x, 0, B, h, w, joi, partials, tiles) != 0 and b"dilation" in lib.quber_last_error()
    blk.dil, blk.c = 2, 96
    assert blk.joint(x, 0, B, h, w, joi, partials, tiles) != 0 and b"64 or 128" in lib.quber_last_error()
    blk.c, blk.r = 64, 9
    out = torch.full((B, h, w, 64), 3.0, device="cuda")
    assert blk.apply(joi, None, 0, out, 0, B, h, w, partials, tiles, None, None) != 0 and b"hidden" in lib.quber_last_error()
    blk.r = 8
    assert blk.apply(joi, x70, 0, out, 0, B, h, w, partials, tiles, None, None) != 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.quber_op_cgnet_sums(_p(joi), 64, B, h, w, 64, _p(partials), 5, st) != 0
    torch.cuda.synchronize()
    assert (joi == 3.0).all() and (out == 3.0).all() and (partials == 0).all()
    # the config check refuses frames that are no multiple of 8
    with pytest.raises(_lib.QuberError, match="multiples of 8"):
        CgnetEngine(cgnet_arch.init_state_dict(0), 60, 72, 1)


# ---- the overlap entry ----
def _overlap(fg, masks, h, w):
    lib = _lib.load()
    B, K = masks.shape[:2]
    counts = torch.full((B, max(K, 1), 2), -5, dtype=torch.int64, device="cuda")
    fg_d, m_d = torch.from_numpy(fg).cuda(), torch.from_numpy(masks).cuda()
    _lib.check(lib.quber_foreground_overlap(_p(fg_d), fg.shape[1], fg.shape[2], _p(m_d) if K else C.c_void_p(0), B, K, h, w, _p(counts),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return counts.cpu().numpy()


def test_foreground_overlap_counts():
    rng = np.random.default_rng(5)
    fg = (rng.random((1, 240, 320)) < 0.4).astype(np.uint8)
    fg[0, 90:150, 40:110] = 0
    fg[0, 90:120, 40:110] = 1                                   # a clean edge at small row 120 = full-size row 240
    sc = synth.make_scene(9, 480, 640, 3)
    masks = np.zeros((1, 5, 480, 640), np.uint8)
    masks[0, :3] = sc["masks"][:3]                              # 0 / 255 bytes
    masks[0, 3, 200:280, 100:200] = 1                           # rows 200..239 on the foreground, 240..279 off: ratio exactly 0.5
    got = _overlap(fg, masks, 480, 640)[0]
    up = G.upsample_nearest(fg[0], 480, 640).astype(bool)
    exp = np.array([[np.sum((m != 0) & up), np.sum(m != 0)] for m in masks[0]])
    assert np.array_equal(got, exp), (got, exp)
    assert exp[4].tolist() == [0, 0] and exp[3].tolist() == [4000, 8000]
    kept, index = filter_masks_uoais(list(masks[0]), got)
    ref_kept, ref_index = G.uoais_filter(list(masks[0]), up)
    assert index.tolist() == ref_index and 3 not in index and 4 not in index
    # K = 0: nothing is written
    assert (_overlap(fg, np.zeros((1, 0, 480, 640), np.uint8), 480, 640) == -5).all()
    # an odd pair, two frames
    fg2 = (rng.random((2, 24, 32)) < 0.5).astype(np.uint8)
    m2 = (rng.random((2, 3, 37, 53)) < 0.3).astype(np.uint8)
    got2 = _overlap(fg2, m2, 37, 53)
    for b in range(2):
        up2 = G.upsample_nearest(fg2[b], 37, 53).astype(bool)
        assert np.array_equal(got2[b], np.array([[np.sum((m != 0) & up2), np.sum(m != 0)] for m in m2[b]]))


def test_cgnet_second_call_overwrites_and_batch_below_capacity():
    h, w = 56, 72
    sd = cgnet_arch.init_state_dict(seed=5)
    sc = [synth.make_scene(s, h, w, 3) for s in (31, 32, 33)]
    d = lambda k, idx: torch.from_numpy(np.stack([sc[i][k] for i in idx])).cuda()
    for fused in (1, 0):
        net = CgnetEngine(sd, h, w, 3, fused=fused)
        a1 = net.logits(d("rgb", [0, 1]), d("depth", [0, 1])).cpu()
        b1 = net.logits(d("rgb", [2]), d("depth", [2])).cpu()
        a2 = net.logits(d("rgb", [0, 1]), d("depth", [0, 1])).cpu()
        c1 = net.logits(d("rgb", [2, 0, 1]), d("depth", [2, 0, 1])).cpu()
        assert torch.equal(a1, a2), "a batch's result depends on the call before it"
        assert not torch.equal(a1[:1], b1)
        x = torch.cat([G.preprocess(sc[i]["rgb"], sc[i]["depth"]) for i in range(3)])
        with torch.no_grad():
            r32 = G.forward(x, _w(sd, torch.float32))
        assert float((a1 - r32[:2]).abs().max()) < TOL and float((b1 - r32[2:]).abs().max()) < TOL and float((c1 - r32[[2, 0, 1]]).abs().max()) < TOL
        net.eng.close()


# ---- the adapter ----
def test_cgnet_predictor_and_initial_filter(tmp_path):
    from PIL import Image
    from quber_amd.eval.refiner_model import MaskRefiner
    z = np.load(golden("cgnet_scene")[0])                        # 240 x 320, seed 0: the synthetic weights CGNet() falls back to
    assert z["rgb"].shape[:2] == (240, 320) and int(z["seed"]) == 0
    with pytest.warns(UserWarning):
        p = CGNet(str(tmp_path / "missing.pth"))
    fg = p.predict_arrays(z["rgb"], z["depth"])
    assert fg.shape == (480, 640) and fg.dtype == np.uint8
    assert (fg == G.upsample_nearest(G.foreground_mask(z["logits"]), 480, 640)).mean() > 0.999
    sc = synth.make_scene(6, 480, 640, 6)
    Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / "rgb.png")
    Image.fromarray((sc["depth"][:, :, 0].astype(np.uint16) * 5 + 300)).save(tmp_path / "depth.png")
    paths = (str(tmp_path / "rgb.png"), str(tmp_path / "depth.png"))
    fg2 = p.predict(*paths)
    assert fg2.shape == (480, 640) and fg2.dtype == np.uint8 and 0 < fg2.mean() < 1
    # the scene's masks, one mask that is all background for the stand-alone predictor, one empty mask
    masks = np.concatenate([sc["masks"] != 0, (fg2 == 0)[None], np.zeros((1, 480, 640), bool)])
    with pytest.warns(UserWarning):
        ref = MaskRefiner(None, None, dataset="OSD", initial_filter="cgnet")
    refined, out, secs, _ = ref.predict(*paths, masks, None)
    up = G.upsample_nearest(out["initial_fg"], 480, 640)
    assert out["initial_fg"].shape == (240, 320)
    exp_kept, exp_index = G.uoais_filter(list(masks), up)
    assert out["initial_keep"].tolist() == exp_index and len(masks) - 1 not in exp_index and len(masks) - 2 not in exp_index and len(exp_index) > 0
    print(f"initial filter kept {exp_index} of {len(masks)} masks")
    # the refiner saw exactly the kept masks: the same call on them, unfiltered, gives the same output
    plain = MaskRefiner(None, None, dataset="OSD")
    none = MaskRefiner(None, None, dataset="OSD", initial_filter=None)
    r0, o0, _, _ = plain.predict(*paths, masks[exp_index], None)
    assert np.array_equal(np.asarray(refined), np.asarray(r0)) and torch.equal(out["sem_seg"], o0["sem_seg"])
    r1, o1, _, _ = plain.predict(*paths, masks, None)
    r2, o2, _, _ = none.predict(*paths, masks, None)
    assert set(o1) == set(o2) and "initial_keep" not in o2
    assert np.array_equal(np.asarray(r1), np.asarray(r2)) and torch.equal(o1["sem_seg"], o2["sem_seg"]) and torch.equal(o1["panoptic_seg"][0], o2["panoptic_seg"][0])
    streamed = list(ref.predict_stream([(paths[0], paths[1], masks)], workers=1))
    assert streamed[0][1]["initial_keep"].tolist() == exp_index
