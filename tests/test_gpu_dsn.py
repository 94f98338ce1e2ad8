"""GPU: the Depth Seeding Network of UOIS-Net-3D (csrc/dsn.hip, csrc/plan_dsn.hip, quber_amd/seeding) against the fixtures generated
from the imported reference module and against the staged restatement tests/dsn_torch.py, for both plans (option key 53: the second
half of an ESP module as one kernel / five convolution launches + esp_merge).

Layer by layer (test_dsn_layers): one forward at batch 3 of a capacity-4 engine (feature_dim 64, 96 x 128) or batch 2 of a capacity-3
engine (every other feature_dim the plan accepts, 32 x 48: LAYER_CASES), then every launch is held to the staged restatement
evaluated in float64 ON THE DEVICE'S OWN INPUTS of that launch.  Bars, from the arithmetic (u = 2^-24):
  pack, max pool, fg     exact: no arithmetic but a sign flip and comparisons
  dense convolutions     max |err| / max(1, max |ref|) < 2e-6, the bar of the exact-fp32 convolution kernels (tests/test_gpu_cgnet.py)
  GroupNorm + ReLU       |err| <= 2e-6 + 1e-5 |ref|, the bar of these kernels in tests/test_gpu_glue.py; the same where the sums come from an
  and x2 bilinear        ESP kernel's tile partials instead of the statistics pass
  ESP, one kernel        output slot of k convolutions (k = 1 for d1 and d2, then 2, 3, 4) plus the residual x:
                         sum over its convolutions of E(d) + (k + 1) u (sum |d| + |x|), E(d) = 2e-6 max(1, max |d|) the dense bar on that
                         convolution: the accumulator carries the running sum, so each convolution adds its own error, and the k - 1
                         hand-overs, the residual add and one store rounding are at most u of the magnitudes summed
  esp_merge              on the five tensors the device wrote: k adds (k - 1 of the running sum, one residual), (k + 1) u (sum |d| + |x|)
  heads                  (C + 1) u sum |w| |f|: a chain of C fused multiply-adds
  votes                  float32(xyz + offsets) of the device's own offsets, to the bit; classes = first maximum of the device's own logits
The stand-alone hooks (test_esp_hooks) hold both ESP kernels on the smallest shapes that still go wrong to the bound of an fmaf chain,
9 n u sum |w| |t| per convolution, on an input with a large constant added: a kernel that pads with anything but zeros of t, or lets a
pad channel of t's stride into the sum, misses that bound by orders of magnitude."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dsn_torch as D
from conftest import golden
from quber_amd import _lib, dsn_arch
from quber_amd.seeding import DsnEngine

pytestmark = pytest.mark.gpu
TOL = 1e-4
U = 2.0 ** -24


def _w(sd, dtype):
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


def _oracle_errors(got, x, sd):
    """per output (logits, offsets): (max |HIP - f64|, max |restatement f32 - f64|) per frame of x, and the float32 restatement"""
    with torch.no_grad():
        r32 = D.forward(x, _w(sd, torch.float32))
        r64 = D.forward(x.double(), _w(sd, torch.float64))
    B = x.shape[0]
    out = []
    for g, a, b in zip(got, r32, r64):
        hip = (g.double() - b).abs().reshape(B, -1).max(1).values.numpy()
        o32 = (a.double() - b).abs().reshape(B, -1).max(1).values.numpy()
        out.append((hip, o32, a))
    return out


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("path", golden("dsn_scene"), ids=os.path.basename)
def test_dsn_golden(path, fused):
    z = np.load(path)
    h, w = z["xyz"].shape[1:]
    sd = dsn_arch.init_state_dict(int(z["seed"]), gain=float(z["gain"]), feature_dim=int(z["feature_dim"]))
    net = DsnEngine(sd, h, w, 3, fused=fused)
    assert net.eng.get_option(53) == fused and net.feature_dim == 64
    x = torch.from_numpy(np.stack([z["xyz"], z["xyz"][:, ::-1].copy()]))              # the scene and its vertical flip
    o = net.run(x.cuda(), logits=True, offsets=True, votes=True, classes=True, fg=True)
    lg, off = o["fg_logits"].cpu(), o["center_offsets"].cpu()
    for name, got, ref in (("fg_logits", lg, z["fg_logits"]), ("center_offsets", off, z["center_offsets"])):
        err = float(np.abs(got[0].numpy() - ref).max())
        print(f"{os.path.basename(path)} fused {fused} {name}: max |HIP - reference f32| {err:.3e} (ref_f32_err {float(z['ref_f32_err']):.3e})")
        assert err < TOL
    for name, got, (hip, o32, r32) in zip(("fg_logits", "center_offsets"), (lg, off), _oracle_errors((lg, off), x, sd)):
        for i in range(2):
            print(f"PARITY-E2E | {os.path.basename(path)} fused {fused} {name} frame {i} | HIP {hip[i]:.3e} | torch-fp32 {o32[i]:.3e} | ratio {hip[i] / o32[i]:.2f}")
        assert float((got[1] - r32[1]).abs().max()) < TOL                            # the flipped frame
        assert (hip <= 2 * o32).all(), (name, hip, o32)
    cls = o["fg_classes"].cpu().numpy()
    agree = (cls[0] == np.argmax(z["fg_logits"], 0)).mean()
    print(f"class agreement {agree:.6f} (near_tie_share {float(z['near_tie_share']):.2e})")
    assert agree > 0.999
    # what the head derives from its own outputs, and the two entry points
    xc = D.clean(x, True)
    assert torch.equal(o["votes"].cpu(), xc + off)
    assert np.array_equal(cls, D.classes(lg).numpy()) and np.array_equal(o["fg"].cpu().numpy(), (cls == 2).astype(np.uint8))
    lg2, off2 = net.forward(x.cuda())
    v2, fg2, cls2 = net.seed(x.cuda())
    assert torch.equal(lg2.cpu(), lg) and torch.equal(off2.cpu(), off) and torch.equal(v2.cpu(), o["votes"].cpu())
    assert torch.equal(fg2.cpu(), o["fg"].cpu()) and torch.equal(cls2.cpu(), o["fg_classes"].cpu())
    net.close()


def _within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                        # a NaN is outside every bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst {ratio:.2f}x, max error {float(err.max()):.3e}"
    return ratio


def _dense(d):
    return 2e-6 * max(1.0, float(d.abs().max()))


def _esp_slots(ds, x):
    """float64 d1, d2, d4, d8, d16 and x -> per output channel (magnitude summed, number of convolutions k, dense bars summed)"""
    mags, ks, es = [ds[0].abs()], [1], [_dense(ds[0])]
    run, e = None, 0.0
    for k, d in enumerate(ds[1:], 1):
        run = d.abs() if run is None else run + d.abs()
        e += _dense(d)
        mags.append(run.clone())
        ks.append(k)
        es.append(e)
    mag = torch.cat(mags, 1) + (0 if x is None else x.abs())
    kk = torch.cat([torch.full((m.shape[1],), float(k)) for m, k in zip(mags, ks)]).double()[None, :, None, None]
    ee = torch.cat([torch.full((m.shape[1],), float(e)) for m, e in zip(mags, es)]).double()[None, :, None, None]
    return mag, kk, ee


# ---- layer by layer ----
class _Forward:
    """one forward at batch n of a capacity-cap engine with every tap read back as float64 NCHW"""

    def __init__(self, h, w, fused, feature_dim=64, n=3, cap=4):
        self.n = n
        self.sd = dsn_arch.init_state_dict(seed=3, feature_dim=feature_dim)
        raw = np.stack([D.synth_xyz(h, w, s) for s in (41, 42, 43)[:n]])
        raw[1, :, : h // 2] = np.nan                                  # one frame with half its pixels missing
        self.raw = torch.from_numpy(raw)
        net = DsnEngine(self.sd, h, w, cap, fused=fused)
        assert net.feature_dim == feature_dim and net.eng.get_option(53) == fused
        o = net.run(self.raw.cuda(), logits=True, offsets=True, votes=True, classes=True, fg=True)
        self.outs = {k: v.cpu() for k, v in o.items()}
        self.plan = net.eng.plan()
        names = {s.out for s in D.plan(fused) if s.out not in D.OUTPUTS} | set(D.CONCAT) | {n + ".conv1.buf" for n in D.ESP}
        self.taps = {k: net.eng.debug_tensor(k, n).cpu() for k in sorted(names)}
        net.close()

    def get(self, name):
        if name == "input":
            return self.raw.double()
        if name in D.OUTPUTS:
            t = self.outs[name]
            return t.double() if t.dtype == torch.float32 else t
        t = self.taps[name].double()                                  # [n,H,W,C]
        if name == "xyz":
            return t.reshape(self.n, 3, -1, t.shape[2])
        return t.permute(0, 3, 1, 2)


# (h, w, feature_dim, fused, batch, capacity).  96 x 128 at 64 as ever; then every other feature_dim the plan accepts on 32 x 48 frames: the
# one-kernel form (key 53 = 1) at each - with 64 that executes esp_branches_kernel<NT> for every NT in 1..13 - and the five convolution
# launches + esp_merge at 8, 12 (no multiple of 8), 20 (n == n1, whole K slices: the row-skipping dilated route), 44 and 60
LAYER_CASES = [(96, 128, 64, 1, 3, 4), (96, 128, 64, 0, 3, 4)] + [(32, 48, fd, 1, 2, 3) for fd in range(8, 64, 4)] + [(32, 48, fd, 0, 2, 3) for fd in (8, 12, 20, 44, 60)]
LAYER_IDS = ["fused", "unfused"] + [f"fd{fd}-{'fused' if f else 'unfused'}-{h}x{w}" for h, w, fd, f, _, _ in LAYER_CASES[2:]]


@pytest.mark.parametrize("h,w,feature_dim,fused,n,cap", LAYER_CASES, ids=LAYER_IDS)
def test_dsn_layers(h, w, feature_dim, fused, n, cap):
    """96 x 128: the ESP modules run on 24 x 32, 12 x 16 and 6 x 8 maps - on the last only the centre taps of d8 and d16 fall inside the
    map, on the second d16 reaches in from neither side; 24 * 32 = 768 pixels are 12 tiles, 6 * 8 = 48 less than one.
    32 x 48, batch 2 of 3: the ESP modules run on 8 x 12, 4 x 6 and 2 x 3 maps - 96 pixels are a tile and a half, 24 and 6 less than one;
    on the smallest map dilation 4, 8 and 16 reach only the centre tap.  The width decides the ESP split (n1 + 4 n, the kernel instance
    NT = ceil(n1 / 16), pad channels of t or none) and the route of every convolution (Cin % 32, Cout % 32, Cin < 128)."""
    fd = feature_dim
    fw = _Forward(h, w, fused, fd, n, cap)
    sd = fw.sd
    w64 = _w(sd, torch.float64)
    steps = D.plan(bool(fused))
    failures, kinds = [], {}
    for st in steps:
        ins = [i.take(fw.get) for i in st.ins]
        got = fw.get(st.out)
        with torch.no_grad():
            ref = st.fn(w64, *ins)
        assert got.shape == ref.shape, st.out
        note = ""
        e_hip = float((got.double() - ref.double()).abs().max())
        try:
            if st.kind in ("pack", "pack8", "pool", "classes", "fg"):
                assert torch.equal(got, ref), st.out
                if st.kind in ("pack", "pack8"):
                    assert torch.equal(torch.signbit(got), torch.signbit(ref)), st.out + ": the sign of a zero"
                note = "exact"
            elif st.kind == "conv":
                rel = e_hip / max(1.0, float(ref.abs().max()))
                note = f"rel {rel:.2e} of 2e-6"
                assert rel < 2e-6, f"{st.out}: {rel:.3e}"
            elif st.kind in ("gn", "bilinear"):
                ratio = _within(got, ref, 2e-6 + 1e-5 * ref.abs(), st.out)
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "esp":
                with torch.no_grad():
                    ds = [D.conv(ins[0], w64, f"{st.key}.dilated{d}", d) for d in dsn_arch.DILATIONS]
                mag, kk, ee = _esp_slots(ds, ins[1])
                ratio = _within(got, ref, ee + (kk + 1) * U * mag, st.out)
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "merge":
                mag, kk, _ = _esp_slots(ins[:5], ins[5])
                ratio = _within(got, ref, (kk + 1) * U * mag, st.out)
                note = f"{ratio:.2f} of the bound"
            elif st.kind == "head":
                wk = w64[st.key + ".weight"]
                ratio = _within(got, ref, (wk.shape[1] + 1) * U * F.conv2d(ins[0].abs(), wk.abs()), st.out)
                note = f"{ratio:.2f} of the bound"
            else:
                assert st.kind == "votes"
                assert torch.equal(got.float(), ins[0].float() + ins[1].float()), st.out
                note = "exact"
        except AssertionError as ex:
            failures.append(str(ex))
            note += " FAILED"
        kinds[st.kind] = kinds.get(st.kind, 0) + 1
        print(f"PARITY-OP | {h}x{w} fd {fd} fused {fused} | {st.op} | {st.out} | {st.kind} | HIP {e_hip:.3e} | {note}")
    assert not failures, "\n".join(failures)
    # the plan's ops are the restatement's, in order and under the same names
    assert [n for n, _, _, _ in fw.plan] == D.ops(bool(fused))
    assert len(fw.plan) == (52 if fused else 67)
    assert kinds.get("esp", 0) == (3 if fused else 0) and kinds.get("merge", 0) == (0 if fused else 3) and kinds["gn"] == 19 and kinds["pool"] == 4
    assert kinds["conv"] == 20 + (0 if fused else 15) and kinds["bilinear"] == 4
    # a concatenation buffer holds exactly its two halves; the channels of t's stride behind the real ones are still exactly zero
    for name, parts in D.CONCAT.items():
        assert torch.equal(fw.get(name), torch.cat([fw.get(p) for p in parts], 1)), name
    for name, c in zip(D.ESP, (4 * fd, 8 * fd, 16 * fd)):
        nn, n1 = dsn_arch.esp_split(c)
        buf = fw.taps[name + ".conv1.buf"]
        assert buf.shape[3] == 16 * ((n1 + 15) // 16) and buf.shape[3] >= nn, name        # (fd 20 and 40: n == n1 == the stride, no pad channels)
        assert (buf[..., nn:].numpy().view(np.uint32) == 0).all(), f"{name}: pad channels {nn}.. of t were written"
        assert float(buf[..., :nn].abs().max()) > 0, name
    assert fw.get("X").shape[1] == 8
    # end to end, every frame
    lg, off = fw.outs["fg_logits"], fw.outs["center_offsets"]
    for name, got, (hip, o32, r32) in zip(("fg_logits", "center_offsets"), (lg, off), _oracle_errors((lg, off), fw.raw, sd)):
        assert float((got - r32).abs().max()) < TOL
        for i in range(n):
            print(f"PARITY-E2E | batch {n} of {cap}, {h}x{w} fd {fd} fused {fused} {name} frame {i} | HIP {hip[i]:.3e} | torch-fp32 {o32[i]:.3e} | ratio {hip[i] / o32[i]:.2f}")
        assert (hip <= 2 * o32).all(), (name, hip, o32)


# ---- the stand-alone hooks ----
def _p(t, elems=0):
    return C.c_void_p(t.data_ptr() + 4 * elems if t is not None else 0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _view(rng, B, h, w, c, cs, c0, fill):
    """a [B,h,w,cs] host buffer filled with `fill`, random data in channels c0 .. c0 + c -> (buffer, the data as NCHW float64)"""
    buf = np.full((B, h, w, cs), fill, np.float32)
    data = rng.standard_normal((B, h, w, c)).astype(np.float32)
    buf[..., c0:c0 + c] = data
    return buf, torch.from_numpy(data).double().permute(0, 3, 1, 2)


ESP_CASES = [(20, 20, 36), (64, 20, 36), (256, 20, 36), (20, 6, 8), (64, 6, 8), (256, 6, 8),
             (128, 20, 36), (128, 6, 8), (192, 20, 36), (640, 6, 8), (960, 6, 8)]
ESP_GROUPS = {20: 10, 64: 64, 256: 64, 128: 64, 192: 48, 640: 40, 960: 60}          # norm groups: a divisor of C, at most 64


@pytest.mark.parametrize("c,h,w", ESP_CASES, ids=[f"c{c}-{h}x{w}" for c, h, w in ESP_CASES])
def test_esp_hooks(c, h, w):
    """20 x 36: dilation 16 reaches into the map from both sides in both axes (rows 0..3 and 16..19 see a tap 16 rows away), 720 pixels
    are 11 tiles and a quarter; 6 x 8: only the centre taps of d8 / d16 fall inside, 48 pixels are three waves of one tile.  C = 20
    (n = n1 = 4), 64 (12 / 16), 256 (51 / 52: t on a stride of 64 + 8 behind 4 foreign channels, the channels 51.. holding 1e3).  Batch 2
    of capacity 3; the module's input and output are channel slices of wider buffers.  C = 128 (25 / 28) and 192 (38 / 40) run the kernel
    instances NT = 2 and 3, 640 (128 / 128) and 960 (192 / 192) NT = 8 and 12 with n == n1 a multiple of 16: t has no pad channels, the
    first foreign one follows the last real one."""
    lib = _lib.load()
    rng = np.random.default_rng(c * 1000 + h)
    n, n1 = dsn_arch.esp_split(c)
    groups = ESP_GROUPS[c]
    assert c % groups == 0 and groups <= 64 and lib.quber_op_esp_kernel(n1) == (n1 + 15) // 16
    B, cap = 2, 3
    nt16 = 16 * ((n1 + 15) // 16)
    t_cs, t_c0 = nt16 + 12, 4
    tbuf, t = _view(rng, cap, h, w, n, t_cs, t_c0, 1e3)
    tbuf[..., t_c0:t_c0 + n] += 40.0                                   # the large constant
    t = t + 40.0
    xbuf, x = _view(rng, cap, h, w, c, c + 8, 8, -7.0)
    ws = [(rng.standard_normal((n1 if i == 0 else n, n, 3, 3)) * np.sqrt(2.0 / (9 * n))).astype(np.float32) for i in range(5)]
    w64 = [torch.from_numpy(a).double() for a in ws]
    with torch.no_grad():
        ds = [F.conv2d(t, wk, None, 1, d, d) for wk, d in zip(w64, dsn_arch.DILATIONS)]
        ref = D.esp_combine(ds, x)
        # an fmaf chain over the 9 n products of a convolution: 9 n u sum |w| |t|
        chain = [9 * n * U * F.conv2d(t.abs(), wk.abs(), None, 1, d, d) for wk, d in zip(w64, dsn_arch.DILATIONS)]
    mag, kk, _ = _esp_slots(ds, x)
    bound = D.esp_combine(chain) + (kk + 1) * U * mag
    o_cs, o_c0 = c + 12, 4
    tiles = lib.quber_op_esp_tiles(h, w)
    assert tiles == (h * w + 63) // 64
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    td, xd, wd = dev(tbuf), dev(xbuf), [dev(a) for a in ws]
    packed = torch.empty(lib.quber_op_esp_packed_floats(n1), dtype=torch.float32, device="cuda")
    _lib.check(lib.quber_op_esp_pack(*[_p(a) for a in wd], n, n1, _p(packed), _st()))

    def run(which, first_fill):
        out = torch.full((cap, h, w, o_cs), first_fill, dtype=torch.float32, device="cuda")
        parts = torch.full((cap, tiles, groups, 2), -1.0, dtype=torch.float64, device="cuda")
        stats = torch.full((cap, groups, 2), -1.0, dtype=torch.float64, device="cuda")
        res = []
        for _ in range(2):                                             # the second call overwrites the first
            if which == "branches":
                rc = lib.quber_op_esp_branches(_p(td, t_c0), t_cs, _p(xd, 8), c + 8, _p(out, o_c0), o_cs, B, h, w, c, groups, _p(packed), _p(parts), tiles, _st())
            else:
                rc = lib.quber_op_esp_merge(_p(dd[0], 4), n1 + 8, *[_p(a, 4) for a in dd[1:]], n + 8, _p(xd, 8), c + 8, _p(out, o_c0), o_cs, B, h, w, c,
                                            groups, _p(parts), tiles, _st())
            _lib.check(rc)
            _lib.check(lib.quber_op_esp_stats(_p(parts), B, tiles, groups, _p(stats), _st()))
            res.append((out.cpu().clone(), parts.cpu().clone(), stats.cpu().clone()))
        (o1, p1, s1), (o2, p2, s2) = res
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)), which
        assert torch.equal(p1.view(torch.int64), p2.view(torch.int64)) and torch.equal(s1.view(torch.int64), s2.view(torch.int64)), f"{which}: sums differ between two runs"
        # nothing outside the view of the first two frames was written
        assert (o1[:B, :, :, :o_c0] == first_fill).all() and (o1[:B, :, :, o_c0 + c:] == first_fill).all() and (o1[B:] == first_fill).all(), which
        assert (p1[B:] == -1.0).all() and (s1[B:] == -1.0).all(), which
        got = o1[:B, :, :, o_c0:o_c0 + c].double().permute(0, 3, 1, 2)
        # the sums are those of what was stored: float64 sums of float32 values in another order, |err| <= pixels * 2^-52 * sum |v| (|v|^2)
        g = got.reshape(B, groups, -1)
        for k, (v, name) in enumerate(((g, "sums"), (g * g, "sums of squares"))):
            tot = v.sum(2)
            assert ((s1[:B, :, k] - tot).abs() <= g.shape[2] * 2.0 ** -52 * v.abs().sum(2)).all(), f"{which}: {name}"
        return got

    got = run("branches", 5.0)
    ratio = _within(got, ref[:B], bound[:B], f"esp_branches c {c} {h}x{w}")
    print(f"PARITY-HOOK | esp_branches | c {c} n {n} n1 {n1} {h}x{w} | max error {float((got - ref[:B]).abs().max()):.3e} | {ratio:.3f} of the bound | max |ref| {float(ref.abs().max()):.1f}")
    # esp_merge on float32 convolutions of its own (torch, rounded): k adds, to the u bound
    dd, d32 = [], []
    for i, d in enumerate(ds):
        co = n1 if i == 0 else n
        buf = np.full((cap, h, w, co + 8), 3e3, np.float32)
        buf[..., 4:4 + co] = d.permute(0, 2, 3, 1).numpy().astype(np.float32)
        dd.append(dev(buf))
        d32.append(torch.from_numpy(buf[..., 4:4 + co]).double().permute(0, 3, 1, 2))
    refm = D.esp_combine(d32, x)
    magm, kkm, _ = _esp_slots(d32, x)
    gotm = run("merge", -9.0)
    ratio = _within(gotm, refm[:B], ((kkm + 1) * U * magm)[:B], f"esp_merge c {c} {h}x{w}")
    print(f"PARITY-HOOK | esp_merge | c {c} {h}x{w} | max error {float((gotm - refm[:B]).abs().max()):.3e} | {ratio:.3f} of the bound")
    # refused views launch nothing
    assert lib.quber_op_esp_branches(_p(td, t_c0), nt16 - 4, _p(xd, 8), c + 8, _p(td), o_cs, B, h, w, c, groups, _p(packed), _p(packed), tiles, _st()) != 0
    assert lib.quber_op_esp_branches(_p(td, t_c0), t_cs, _p(xd, 8), c + 8, _p(td), o_cs, B, h, w, c, groups, _p(packed), _p(packed), tiles + 1, _st()) != 0
    assert lib.quber_op_esp_merge(_p(dd[0], 4), n1 - 1, *[_p(a, 4) for a in dd[1:]], n + 8, _p(xd, 8), c + 8, _p(td), o_cs, B, h, w, c, groups, _p(packed), tiles, _st()) != 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", [64, 128])
def test_groupnorm_64_groups(c):
    """launch_gn_stats / launch_gn_apply as the plan calls them: 64 groups of 1 and of 2 channels, into a channel slice"""
    lib = _lib.load()
    rng = np.random.default_rng(c)
    B, h, w, groups = 2, 9, 13, 64
    x = (rng.standard_normal((B, h, w, c)) * 2 + 3).astype(np.float32)
    gam, bet = rng.uniform(0.6, 1.4, c).astype(np.float32), rng.normal(0, 0.1, c).astype(np.float32)
    xd, gd, bd = (torch.from_numpy(a).cuda() for a in (x, gam, bet))
    out = torch.full((B, h, w, 2 * c), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.full((B, groups, 2), 1e9, dtype=torch.float64, device="cuda")
    _lib.check(lib.quber_op_gn_stats(_p(xd), c, 0, 4, B, h, w, c, 1, groups, _p(stats), 1, _st()))
    _lib.check(lib.quber_op_gn_apply(_p(xd), c, 0, 4, _p(out, c), 2 * c, 0, 4, B, h, w, c, 1, groups, _p(stats), _p(gd), _p(bd), c, C.c_float(1e-5), 1, _st()))
    x64 = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    ref = F.relu(F.group_norm(x64, groups, torch.from_numpy(gam).double(), torch.from_numpy(bet).double(), 1e-5))
    o = out.cpu()
    assert (o[..., :c] == 7.0).all()
    ratio = _within(o[..., c:].double().permute(0, 3, 1, 2), ref, 2e-6 + 1e-5 * ref.abs(), f"groupnorm {c} channels in 64 groups")
    g = x64.reshape(B, groups, -1)
    s = stats.cpu()
    assert ((s[..., 0] - g.sum(2)).abs() <= 1e-12 * g.abs().sum(2)).all() and ((s[..., 1] - (g * g).sum(2)).abs() <= 1e-12 * (g * g).sum(2)).all()
    print(f"PARITY-HOOK | groupnorm | {c} channels, 64 groups | {ratio:.3f} of the bound")


@pytest.mark.parametrize("flags", [0, 1])
def test_dsn_pack_hook(flags):
    lib = _lib.load()
    rng = np.random.default_rng(7)
    B, h, w = 2, 5, 11                                                 # 110 pixels: not a multiple of anything
    xyz = rng.standard_normal((3, 3, h, w)).astype(np.float32)
    xyz[0, :, 1, 2] = np.nan
    xyz[1, 1, 3, :] = np.nan
    xyz[0, 2, 0, 0] = np.nan
    xyz[1, 1, 0, 0] = 0.0
    xd = torch.from_numpy(xyz).cuda()
    x8 = torch.full((3, h, w, 8), 9.0, dtype=torch.float32, device="cuda")
    cl = torch.full((3, 3, h, w), 9.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.quber_op_dsn_pack(_p(xd), B, h, w, flags, _p(x8), _p(cl), _st()))
    ref = np.where(np.isnan(xyz), np.float32(0), xyz)
    if flags & 1:
        ref[:, 1] *= -1
    x8h, clh = x8.cpu().numpy(), cl.cpu().numpy()
    assert np.array_equal(clh[:B].view(np.uint32), ref[:B].view(np.uint32)) and (clh[B:] == 9.0).all()
    assert np.array_equal(x8h[:B, ..., :3].view(np.uint32), ref[:B].transpose(0, 2, 3, 1).view(np.uint32))
    assert (x8h[:B, ..., 3:].view(np.uint32) == 0).all() and (x8h[B:] == 9.0).all()
    # either destination alone
    cl2 = torch.zeros_like(cl)
    _lib.check(lib.quber_op_dsn_pack(_p(xd), B, h, w, flags, None, _p(cl2), _st()))
    assert torch.equal(cl2[:B].cpu(), cl[:B].cpu())
    assert lib.quber_op_dsn_pack(_p(xd), B, h, w, flags, None, None, _st()) != 0


def test_dsn_head_hook():
    """12 channels on a stride of 16, 3 x 7 pixels, batch 2 of 3.  fg_module's rows 0 and 2 are equal: their logits tie exactly wherever
    they are the maximum, and the class must be 0 - never 2; a pixel of zeros ties all three."""
    lib = _lib.load()
    rng = np.random.default_rng(11)
    B, cap, h, w, c, cs = 2, 3, 3, 7, 12, 16
    fbuf, f = _view(rng, cap, h, w, c, cs, 4, 1e3)
    fbuf[0, 0, 0, 4:4 + c] = 0.0
    f[0, :, 0, 0] = 0.0
    wfg = rng.standard_normal((3, c)).astype(np.float32)
    wfg[2] = wfg[0]
    wcd = rng.standard_normal((3, c)).astype(np.float32)
    clean = rng.standard_normal((cap, 3, h, w)).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fd_, wf, wc, cl = dev(fbuf), dev(wfg), dev(wcd), dev(clean)
    lg, off, vo = (torch.full((cap, 3, h, w), 5.0, dtype=torch.float32, device="cuda") for _ in range(3))
    cls, fg = (torch.full((cap, h, w), 9, dtype=torch.uint8, device="cuda") for _ in range(2))
    _lib.check(lib.quber_op_dsn_head(_p(fd_, 4), cs, B, h, w, c, _p(cl), _p(wf), _p(wc), _p(lg), _p(off), _p(vo), cls.data_ptr(), fg.data_ptr(), _st()))
    lgh, offh, voh, clsh, fgh = (t.cpu() for t in (lg, off, vo, cls, fg))
    for got, wk, name in ((lgh, wfg, "logits"), (offh, wcd, "offsets")):
        wk64 = torch.from_numpy(wk).double()[:, :, None, None]
        _within(got[:B].double(), F.conv2d(f[:B], wk64), (c + 1) * U * F.conv2d(f[:B].abs(), wk64.abs()), "dsn_head " + name)
        assert (got[B:] == 5.0).all()
    assert torch.equal(voh[:B], torch.from_numpy(clean[:B]) + offh[:B]) and (voh[B:] == 5.0).all()
    assert torch.equal(lgh[:B, 0], lgh[:B, 2])                           # the ties are exact
    assert np.array_equal(clsh[:B].numpy(), D.classes(lgh[:B]).numpy()) and not (clsh[:B] == 2).any() and (clsh[:B] == 0).any() and (clsh[:B] == 1).any()
    assert clsh[0, 0, 0] == 0 and (fgh[:B] == 0).all() and (clsh[B:] == 9).all() and (fgh[B:] == 9).all()
    # class 2 where it is the only maximum
    wfg2 = wfg.copy()
    wfg2[2] = -wfg[0] - wfg[1]
    _lib.check(lib.quber_op_dsn_head(_p(fd_, 4), cs, B, h, w, c, None, _p(dev(wfg2)), _p(wc), _p(lg), None, None, cls.data_ptr(), fg.data_ptr(), _st()))
    c2 = D.classes(lg.cpu()[:B]).numpy()
    assert np.array_equal(cls.cpu()[:B].numpy(), c2) and (c2 == 2).any() and np.array_equal(fg.cpu()[:B].numpy(), (c2 == 2).astype(np.uint8))
    assert lib.quber_op_dsn_head(_p(fd_, 4), cs, B, h, w, c, None, _p(wf), _p(wc), _p(lg), None, _p(vo), None, None, _st()) != 0      # votes without xyz


# ---- the predictor ----
SEED_KEYS = {"seeding_fg", "seeding_report"}


def test_predictor_seeding_equals_votes_from_the_host():
    """predict(rgb, depth, xyz=) under seeding= returns, bit for bit, what predict(rgb, depth, center_votes=, fg=) returns when fed the same
    engine's seed() outputs copied to the host, in every key; seeding_fg / seeding_report come on top.  The refiner's forward is the stub of
    tests/test_gpu_masknms.py (fixed logits; it records the encoded initial masks): everything before and after it is the real path."""
    from quber_amd import synth
    from quber_amd.gms import IMP, GaussianMeanShift
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
    from quber_amd.meanshift import MeanShift
    from quber_amd.seeding import DepthSeeding
    from test_gpu_cleanup import speck_logits
    from test_gpu_masknms import _equal, _predictor, dev
    z = np.load([p for p in golden("dsn_scene") if "96x128" in p][0])
    h, w = z["xyz"].shape[1:]
    sd = dsn_arch.init_state_dict(int(z["seed"]), gain=float(z["gain"]))
    logits = speck_logits(h, w)
    sc = [synth.make_scene(3 + b, h, w, 2) for b in range(2)]
    rgb, dep = np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])
    xyz = [z["xyz"], np.ascontiguousarray(z["xyz"][:, :, ::-1])]                       # the scene and its mirror image
    # (seeded weights vote all over the place: a bandwidth of 0.3 m gathers them into a few clusters that survive min_pixels)
    gkw = dict(num_seeds=40, sigma=0.3, epsilon=0.3, min_pixels=100, imp=IMP(5, True), seed=5)
    g1, g2 = GaussianMeanShift(**gkw), GaussianMeanShift(**gkw)
    kw = dict(decode_errors=True, track_initial=True)
    off1, off2 = [], []
    # the checkpoint form of the weights: under 'model', with DataParallel's prefix
    seeding = DepthSeeding({"model": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}})
    seeded = _predictor(h, w, logits, off1, cluster=g1, seeding=seeding, **kw)
    plain = _predictor(h, w, logits, off2, cluster=g2, **kw)
    assert plain.seeding is None

    def host_inputs(frames):
        x = torch.from_numpy(np.stack([xyz[f] for f in frames])).cuda()
        v, f, cls = seeding.engine_for(h, w, len(frames), seeded.device).seed(x)
        return v.cpu().numpy(), f.cpu().numpy(), cls.cpu()

    def check(a, b, cls, what):
        assert set(a) - SEED_KEYS == set(b) and SEED_KEYS <= set(a) and not SEED_KEYS & set(b), (what, sorted(a), sorted(b))
        for key in b:
            _equal(a[key], b[key], "%s: %s" % (what, key))
        assert a["seeding_fg"].dtype == torch.uint8 and torch.equal(a["seeding_fg"].cpu(), cls), what
        assert a["seeding_report"].dtype == torch.int64 and a["seeding_report"].tolist() == [int((cls == k).sum()) for k in range(3)], what
        assert int(a["cluster_report"][5]) == int((cls == 2).sum()) > 0, what         # the clustering saw the network's foreground

    a = seeded.predict(rgb[0], dep[0], xyz=xyz[0].transpose(1, 2, 0))[0]               # [H,W,3], as the reference holds a point cloud
    v, f, cls = host_inputs([0])
    b = plain.predict(rgb[0], dep[0], center_votes=v[0], fg=f[0])[0]
    check(a, b, cls[0], "predict")
    assert int(a["cluster_report"][0]) >= 1, "no cluster survived: the comparison would be empty"
    outs = seeded.predict_batch(rgb, dep, None, xyz=[xyz[1], xyz[0]])                  # [3,H,W]
    v, f, cls = host_inputs([1, 0])
    refs = plain.predict_batch(rgb, dep, None, center_votes=list(v), fg=list(f))
    for i, (a, b) in enumerate(zip(outs, refs)):
        check(a, b, cls[i], "predict_batch frame %d" % i)
    assert len(off1) == len(off2) >= 2
    for x, y in zip(off1, off2):
        assert x.shape == y.shape and torch.equal(x, y)
    # the refusals; none of them has drawn from the clustering's stream
    bare = MaskRefinerPredictor(None, device="cuda:0", seeding=seeding)
    ucn = MaskRefinerPredictor(None, device="cuda:0", seeding=seeding, cluster=MeanShift(num_seeds=8))
    odd = np.zeros((3, 40, 72), np.float32)
    for call in (lambda: plain.predict(rgb[0], dep[0], xyz=xyz[0]),                                                  # without seeding=
                 lambda: seeded.predict(rgb[0], dep[0], xyz=xyz[0], center_votes=v[0], fg=f[0]),
                 lambda: seeded.predict(rgb[0], dep[0], xyz=xyz[0], fg=f[0]),
                 lambda: seeded.predict(rgb[0], dep[0], np.zeros((1, h, w), np.uint8), xyz=xyz[0]),                  # masks
                 lambda: seeded.predict_batch(rgb, dep, [np.zeros((1, h, w), np.uint8)] * 2, xyz=xyz),
                 lambda: seeded.predict_batch(rgb, dep, None, xyz=xyz[:1]),                                          # one cloud for two frames
                 lambda: seeded.predict(rgb[0], dep[0], xyz=xyz[0][:2]),                                             # a wrong shape
                 lambda: seeded.predict(np.zeros((40, 72, 3), np.uint8), np.zeros((40, 72, 3), np.uint8), xyz=odd),  # 40 is no multiple of 16
                 lambda: bare.predict(rgb[0], dep[0], xyz=xyz[0]),                                                   # no cluster=
                 lambda: ucn.predict(rgb[0], dep[0], xyz=xyz[0]),                                                    # the other clusterer
                 lambda: seeded.model.enqueue_batch(dev(rgb), dev(dep), dev(np.zeros((2, 1, h, w), np.uint8)), xyz=xyz)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        MaskRefinerPredictor(None, device="cuda:0", seeding="dsn")
    assert g1.draws([50])[1].tolist() == g2.draws([50])[1].tolist()
    seeding.close()
    for p in (seeded, plain, bare, ucn):
        p.model.close()
