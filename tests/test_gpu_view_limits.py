"""GPU: the convolution kernels right under and right over the view-size gates of their launchers (tests/view_limits.py is the host model and
the case table; tests/test_view_limits_model.py holds its arithmetic).  Views of 1 - 8 GiB: 32-bit byte offsets near their wrap, the
out-of-range constants, the rows past M of the last tile, the fallback kernels' 64-bit paths, outputs above 2^31 and 2^32 bytes on the kernels
without an output gate.

Through the stand-alone ops only.  Operands are filled on the device from a seeded generator and never copied whole; every output lies inside
a larger NaN-filled buffer with a guard of 256 output rows on either side.  Per case and side:
  1. routing - the stage profile where the two sides differ in it, else the model's verdict (asserted) and, over the gate, bit-equal outputs
     with the kernel's own option key on and off;
  2. no NaN left in the output, none gone from the guards;
  3. float64 on the CPU from slices copied with their halos: strips of 16 output rows at the first and last rows, either side of the image
     boundary, and around the input / output elements at byte offsets 2^30, 2^31 - one row, 2^31 and 2^32 where a view reaches them; 256 seeded
     random pixels;
  4. under the gate: the whole output against the kernel the launch would fall back to, inside the bar (case G, which has none: against a
     float64 product computed on the device slice by slice);
  5. the GroupNorm sums against float64 sums of the stored outputs (cases J and L).
Bars, from the tests that hold these kernels: exact fp32 and bf16x3 2e-6 of the output scale (test_conv_igemm_vs_torch, tests/test_gpu_x8.py),
fp16 3e-3 (tests/test_gpu_h8.py), single-kernel Winograd 2e-5 against float64 and 1e-5 against the pipeline (test_conv3x3_winograd_single_kernel).
Figures measured: profiles/view_limits.md."""
import ctypes as C
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import view_limits as vl
from quber_amd import _lib
from test_gpu_h8 import pack
from test_gpu_tile_walks import profiled

pytestmark = pytest.mark.gpu

STRIP = 16
SAMPLES = 256
_P = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bars(g):
    """-> (against float64, against the other kernel), relative to the output scale."""
    return {"f16": (3e-3, 3e-3), "wino": (2e-5, 1e-5)}.get(g.op, (2e-6, 2e-6))


def chunks_of(n, parts=64):
    step = -(-n // parts)
    return [(lo, min(n, lo + step)) for lo in range(0, n, step)]


def count_nan(t):
    flat = t.reshape(-1)
    return sum(int(torch.isnan(flat[lo:hi]).sum()) for lo, hi in chunks_of(flat.numel()))


def max_abs_diff(a, b):
    """max |a - b| in float64 and its index, slice by slice on the device (a NaN counts as infinite)."""
    shape, a, b = tuple(a.shape), a.reshape(-1), b.reshape(-1)
    best, at = -1.0, 0
    for lo, hi in chunks_of(a.numel()):
        d = (a[lo:hi].double() - b[lo:hi].double()).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        i = int(d.argmax())
        if float(d[i]) > best:
            best, at = float(d[i]), lo + i
    return best, tuple(int(v) for v in np.unravel_index(at, shape))


def bit_equal(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    return all(torch.equal(a[lo:hi], b[lo:hi]) for lo, hi in chunks_of(a.numel()))


def stored_sums(y, groups):
    """float64 sums and sums of squares of the stored outputs per (image, norm group), a slice of rows at a time -> [B][groups][2]."""
    out = torch.zeros((y.shape[0], groups, 2), dtype=torch.float64, device=y.device)
    for b in range(y.shape[0]):
        for lo, hi in chunks_of(y.shape[1]):
            yd = y[b, lo:hi].double().reshape(-1, groups, y.shape[-1] // groups)
            out[b, :, 0] += yd.sum((0, 2))
            out[b, :, 1] += (yd * yd).sum((0, 2))
    return out


class Guarded:
    """An output [B][oh][ow][cout] inside a NaN-filled buffer, GUARD_ROWS output rows of guard on either side."""

    def __init__(self, g, dtype):
        oh, ow = vl.out_size(g)
        self.guard = vl.GUARD_ROWS * g.cout
        n = g.B * oh * ow * g.cout
        self.buf = torch.full((n + 2 * self.guard,), float("nan"), dtype=dtype, device="cuda")
        self.y = self.buf[self.guard:self.guard + n].view(g.B, oh, ow, g.cout)

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.guard]).all()) and bool(torch.isnan(self.buf[-self.guard:]).all())


class Launch:
    """The operands of one geometry on the device (seeded), small ones also on the CPU in float64, and the call of its stand-alone op."""

    def __init__(self, c, g):
        self.c, self.g = c, g
        self.lib = _lib.load()
        gen = torch.Generator(device="cuda").manual_seed(9000 + sum(ord(ch) for ch in c.id) + g.H)
        dt = torch.float16 if g.op == "f16" else torch.float32
        self.dt = dt
        oh, ow = vl.out_size(g)
        rnd = lambda *shape: torch.randn(shape, device="cuda", generator=gen, dtype=dt)
        self.x = rnd(g.B, g.H, g.W, g.cin)
        self.x2 = rnd(g.B, g.H, g.W, g.cin2) if g.op == "dual" else None
        kk = g.cin + g.cin2 if g.op == "dual" else g.cin * g.k * g.k
        w = torch.randn((g.cout, g.cin + g.cin2, g.k, g.k), device="cuda", generator=gen) / kk ** 0.5
        self.scale = torch.rand(g.cout, device="cuda", generator=gen) + 0.5
        if g.groups:        # one sign per norm group, |shift| >= 0.5: no group's mean is near zero, the relative bar of the sums governs
            cpg = g.cout // g.groups
            sign = (1.0 - 2.0 * (torch.arange(g.groups, device="cuda") % 2)).repeat_interleave(cpg)
            self.shift = sign * (0.5 + 0.5 * torch.rand(g.cout, device="cuda", generator=gen))
        else:
            self.shift = torch.randn(g.cout, device="cuda", generator=gen)
        self.res = rnd(g.B, oh, ow, g.cout) if g.residual else None
        if g.op == "dual":
            self.scale = torch.ones(g.cout, device="cuda")
            self.w = w.reshape(g.cout, kk).contiguous()
        elif g.op == "f16":
            w = w.half()
            self.w = pack(w.cpu(), g.kmode).cuda()
        else:
            self.w = w.contiguous()
        self.w64 = w.double().cpu()
        self.scale64, self.shift64 = self.scale.double().cpu(), self.shift.double().cpu()
        self.packed = torch.empty(g.cout * vl.kpad(g), device="cuda") if g.op == "conv2d" else None
        if g.op == "wino":
            self.u = torch.empty(36 * g.cout * g.cin, device="cuda")
            self.ws = torch.empty(36 * vl.wino_tiles(g) * (g.cin + g.cout) + 36 * g.cout * g.cin, device="cuda")
        torch.cuda.synchronize()

    def call(self, out):
        """-> (return code, GroupNorm sums or None); out: a Guarded."""
        g, lib, y = self.g, self.lib, out.y
        oh, ow = vl.out_size(g)
        sums = None
        if g.op == "conv2d":
            rc = lib.quber_op_conv2d(_P(self.x), g.B, g.H, g.W, g.cin, _P(self.w), g.cout, g.k, g.stride, g.pad, g.dil, _P(self.scale), _P(self.shift),
                                     _P(self.res), int(g.relu), _P(self.packed), _P(y), _stream())
        elif g.op == "f16":
            sums = torch.zeros((g.B, g.groups, 2), dtype=torch.float64, device="cuda") if g.groups else None
            rc = lib.quber_op_conv2d_f16(_P(self.x), g.B, g.H, g.W, g.cin, _P(self.w), g.cout, g.k, g.stride, g.pad, g.dil, g.kmode, _P(self.scale),
                                         _P(self.shift), _P(self.res), int(g.relu), _P(sums), g.groups, _P(y), _stream())
        elif g.op == "dual":
            rc = lib.quber_op_conv1x1_dual(_P(self.x), _P(self.x2), g.B, oh, ow, g.cin, g.H, g.W, g.cin2, 1, _P(self.w), _P(self.shift), _P(self.scale),
                                           g.cout, int(g.relu), _P(y), _stream())
        else:
            rc = lib.quber_op_conv3x3_winograd(_P(self.x), g.B, g.H, g.W, g.cin, _P(self.w), g.cout, g.dil, 4, _P(self.scale), _P(self.shift), int(g.relu),
                                               _P(self.u), _P(self.ws), self.ws.numel(), _P(y), _stream())
        torch.cuda.synchronize()
        return rc, sums

    # ---- float64 on the CPU ----
    def _epilogue(self, acc, res):
        """acc: [..., cout] float64."""
        ref = acc * self.scale64 + self.shift64
        if res is not None:
            ref = ref + res.double().cpu()
        return ref.clamp_min(0) if self.g.relu else ref

    def strip(self, b, r0):
        """The float64 reference of output rows [r0, r0 + STRIP) of image b, from the input rows they read -> [rows][ow][cout]."""
        g = self.g
        oh, _ = vl.out_size(g)
        r1 = min(oh, r0 + STRIP)
        res = self.res[b, r0:r1] if self.res is not None else None
        if g.op == "dual":
            mid = g.cin
            acc = self.x[b, r0:r1].double().cpu() @ self.w64[:, :mid, 0, 0].T + self.x2[b, r0:r1].double().cpu() @ self.w64[:, mid:, 0, 0].T
            return self._epilogue(acc, res)
        lo = r0 * g.stride - g.pad
        hi = (r1 - 1) * g.stride - g.pad + g.dil * (g.k - 1) + 1
        xs = self.x[b, max(lo, 0):min(hi, g.H)].double().cpu().permute(2, 0, 1)[None]
        xs = F.pad(xs, (0, 0, max(0, -lo), max(0, hi - g.H)))
        acc = F.conv2d(xs, self.w64, None, g.stride, (0, g.pad), g.dil)[0].permute(1, 2, 0)
        return self._epilogue(acc, res)

    def samples(self, n=SAMPLES):
        """n seeded random output pixels -> (index arrays b, oy, ox; their float64 reference [n][cout])."""
        g = self.g
        oh, ow = vl.out_size(g)
        rng = np.random.default_rng(77 + g.H)
        dev = self.x.device
        b, oy, ox = (torch.from_numpy(rng.integers(0, hi, n)).to(dev) for hi in (g.B, oh, ow))
        res = self.res[b, oy, ox] if self.res is not None else None
        if g.op == "dual":
            mid = g.cin
            acc = self.x[b, oy, ox].double().cpu() @ self.w64[:, :mid, 0, 0].T + self.x2[b, oy, ox].double().cpu() @ self.w64[:, mid:, 0, 0].T
            return (b, oy, ox), self._epilogue(acc, res)
        t = torch.arange(g.k, device=dev) * g.dil
        iy = (oy * g.stride - g.pad)[:, None, None] + t[None, :, None]                   # [n][k][1]
        ix = (ox * g.stride - g.pad)[:, None, None] + t[None, None, :]                   # [n][1][k]
        ok = (iy >= 0) & (iy < g.H) & (ix >= 0) & (ix < g.W)                             # [n][k][k]
        win = self.x[b[:, None, None], iy.clamp(0, g.H - 1), ix.clamp(0, g.W - 1)]       # [n][k][k][cin]
        win = (win * ok[..., None]).double().cpu()
        acc = torch.einsum("nyxc,ocyx->no", win, self.w64)
        return (b, oy, ox), self._epilogue(acc, res)


def strips_of(c, g):
    """(image, first row) of the strips of STRIP output rows: the first rows of image 0, the last rows of the last image, both sides of every
    image boundary, and the rows around the input / output elements at byte offsets 2^30, 2^31 - one row, 2^31 and 2^32 of every view that
    reaches them (an input row iy is read by the output rows around iy / stride)."""
    oh, ow = vl.out_size(g)
    last = max(0, oh - STRIP)
    out = [(0, 0), (g.B - 1, last)]
    for b in range(1, g.B):
        out += [(b - 1, last), (b, 0)]
    per_pixel = [(g.cin * vl.es(g), g.H, g.W, g.stride), (g.cout * vl.es(g), oh, ow, 1)]
    if g.op == "dual":
        per_pixel.append((g.cin2 * 4, g.H, g.W, 1))
    for pp, h, w, stride in per_pixel:
        total = g.B * h * w * pp
        for off in (1 << 30, (1 << 31) - w * pp, 1 << 31, 1 << 32):
            if off < total:
                b, row = divmod(off // pp // w, h)
                r0 = min(last, max(0, row // stride - STRIP // 2))
                if not any(bb == b and abs(r0 - rr) < STRIP // 4 for bb, rr in out):
                    out.append((b, r0))
    return out


def float64_error(launch, y):
    """-> (largest |y - float64| over the strips and the samples, where, the largest |float64| seen: the output scale)."""
    worst, at, scale = -1.0, None, 1.0
    for b, r0 in strips_of(launch.c, launch.g):
        ref = launch.strip(b, r0)
        d = (y[b, r0:r0 + ref.shape[0]].double().cpu() - ref).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        scale = max(scale, float(ref.abs().max()))
        if float(d.max()) > worst:
            i = np.unravel_index(int(d.argmax()), tuple(d.shape))
            worst, at = float(d.max()), (b, r0 + int(i[0]), int(i[1]), int(i[2]))
    (b, oy, ox), ref = launch.samples()
    d = (y[b, oy, ox].double().cpu() - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    scale = max(scale, float(ref.abs().max()))
    if float(d.max()) > worst:
        i = np.unravel_index(int(d.argmax()), tuple(d.shape))
        worst, at = float(d.max()), (int(b[i[0]]), int(oy[i[0]]), int(ox[i[0]]), int(i[1]))
    return worst, at, scale


def whole_output_error_1x1(launch, y):
    """A 1x1 launch without another kernel to compare with (case G): every output element against float64 on the DEVICE, slice by slice."""
    g = launch.g
    x, y = launch.x.reshape(-1, g.cin), y.reshape(-1, g.cout)
    w, scale, shift = (t_.cuda() for t_ in (launch.w64[:, :, 0, 0].T.contiguous(), launch.scale64, launch.shift64))
    worst = -1.0
    for lo, hi in chunks_of(x.shape[0]):
        ref = (x[lo:hi].double() @ w) * scale + shift
        d = (y[lo:hi].double() - (ref.clamp_min(0) if g.relu else ref)).abs()
        worst = max(worst, float(torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d).max()))
    return worst


def set_keys(lib, keys):
    for key, v in keys.items():
        lib.quber_set_tuning(key, v)


def launches(stages):
    return {s: n for s, n in stages.items() if n}


def run_case(cid, side):
    c = vl.BY_ID[cid]
    g = c.under if side == "under" else c.over
    lib = _lib.load()
    dtype = vl.dtype_of(c)
    # the model's verdict and the routing preconditions, for this device's CU count
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bad = [name for name, ok in vl.preconditions(c, g, cus).items() if not ok]
    assert not bad, (cid, side, bad)
    verdict = vl.taken(c.row, g, dtype)
    if cid == "G":
        assert not verdict and not vl.taken("persistent", g)
    else:
        assert verdict == (side == "under"), (cid, side, vl.refusing(c.row, g, dtype))
    need = vl.footprint(c, g)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"case {cid} {side}: {need / vl.GIB:.1f} GiB needed, {free / vl.GIB:.1f} GiB free")
    rel64, rel_other = bars(g)
    t0 = time.perf_counter()
    touched = set(c.keys) | ({c.off[0]} if c.off else set())
    launch = out = other = None
    try:
        launch = Launch(c, g)
        out = Guarded(g, launch.dt)
        set_keys(lib, c.keys)
        (rc, sums), stages = profiled(lambda: launch.call(out))
        stages = launches(stages)
        if c.row == "dual" and side == "over":
            # the stand-alone op has no other kernel to go to: an error, and the output untouched
            assert rc != 0 and "not covered" in lib.quber_last_error().decode(), (rc, lib.quber_last_error())
            assert count_nan(out.buf) == out.buf.numel()
            print(f"view limits {cid} {side}: {c.view} {vl.binding_bytes(c, g)} B refused ({lib.quber_last_error().decode()}) {time.perf_counter() - t0:.1f} s")
            return
        _lib.check(rc)
        # 1. routing by stage
        stage = c.stage if side == "under" else c.stage_over
        assert stages.get(stage, 0) >= 1, (cid, side, stages)
        if c.stage_over and c.stage_over != c.stage:
            absent = c.stage_over if side == "under" else c.stage
            assert not stages.get(absent), (cid, side, stages)
        # 2. finite, guards untouched
        assert count_nan(out.y) == 0, (cid, side, "NaN left in the output")
        assert out.guards_intact(), (cid, side, "a guard was written")
        # 3. float64
        e64, at, scale = float64_error(launch, out.y)
        tol64, tol_other = rel64 * scale, rel_other * scale
        # 4. the other kernel
        ab, at_ab, stages0, equal = None, None, {}, None
        if c.off or c.row == "dual":
            other = Guarded(g, launch.dt)
            if c.off:
                lib.quber_set_tuning(*c.off)
            else:                           # the dual cases: exact fp32 on the persistent kernel against bf16x3 on the x8 kernel
                twin = vl.BY_ID["Dx" if cid == "D" else "D"]
                touched |= set(twin.keys)
                set_keys(lib, {k: vl.DEFAULTS[k] for k in c.keys})
                set_keys(lib, twin.keys)
            (rc0, sums0), stages0 = profiled(lambda: launch.call(other))
            stages0 = launches(stages0)
            _lib.check(rc0)
            assert count_nan(other.y) == 0 and other.guards_intact(), (cid, side, "the other kernel")
            ab, at_ab = max_abs_diff(out.y, other.y)
            if side == "over":
                equal = bit_equal(out.y, other.y)
        elif g.k == 1 and not g.residual:
            ab = whole_output_error_1x1(launch, out.y)         # (asserted below, against the float64 bar: the two are equal in fp32)
        gn = ""
        if g.groups:
            exp = stored_sums(out.y, g.groups)
            mean = float(exp[..., 0].abs().min()) / (out.y[0].numel() // g.groups)
            gn = f" sums: abs {float((sums - exp).abs().max()):.3e} rel {float(((sums - exp).abs() / exp.abs()).max()):.3e} least |mean| {mean:.3f}"
        secs = time.perf_counter() - t0
        print(f"view limits {cid} {side}: {c.view} {vl.binding_bytes(c, g)} B stages {stages} / {stages0} err64 {e64:.3e} at {at} bar {tol64:.3e} "
              f"other {ab if ab is None else format(ab, '.3e')} bar {tol_other:.3e} equal {equal}{gn} {secs:.1f} s")
        assert e64 < tol64, (cid, side, e64, tol64, at)
        if ab is not None:
            if side == "under":
                assert ab < tol_other, (cid, side, ab, tol_other, at_ab)
                if c.off and c.stage_over != c.stage:           # the other kernel really was another one
                    assert not stages0.get(c.stage) and (c.stage_over is None or stages0.get(c.stage_over, 0) >= 1), (cid, stages0)
            else:
                # after the gate it is the same kernel either way
                assert equal, (cid, side, "the launch over the gate differs with the kernel's key on and off", ab, at_ab)
        if g.groups:
            assert mean > 0.05, (cid, side, mean)
            wrong = ~torch.isclose(sums, exp, rtol=2e-6, atol=1e-4)
            assert not bool(wrong.any()), (cid, side, gn, wrong.nonzero()[:8].tolist())
    finally:
        for key in touched:
            lib.quber_set_tuning(key, vl.DEFAULTS[key])
        del launch, out, other
        torch.cuda.empty_cache()


@pytest.mark.parametrize("cid", [c.id for c in vl.CASES])
def test_under_the_gate(cid):
    run_case(cid, "under")


@pytest.mark.parametrize("cid", [c.id for c in vl.CASES if c.over is not None])
def test_over_the_gate(cid):
    run_case(cid, "over")
