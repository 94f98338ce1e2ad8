"""GPU: every launcher of csrc/lmff.hip on its own (the quber_op_lmff_* hooks and quber_foreground_filter), in its one-channel and its
four-channel form, on channel slices of wider buffers, in the second trip of its grid-stride loop (more than 4096 x 256 work items) and
in every refusal, against float64 references.

Every buffer has one frame more than the launch covers and is filled with NaN outside the view: a source's neighbouring channels must
not be read (a NaN would surface), a destination's bytes outside the written slice must come back unchanged.  Scale, shift and slope
differ per channel (slopes of both signs, |slope| <= 0.5), so a vector read at the neighbouring channel shows.

Bounds, from the arithmetic, per element (u = 2^-24, the unit roundoff; m = |a| + |b| or sum |x w|):
  BN + PReLU        3 u m |scale| + u |shift|.  The addition: u m |scale|; y = fma(.., scale, shift): u |y| <= u (m |scale| + |shift|); the
                    negative branch multiplies by the slope and rounds again: the two roundings of y become 2 |slope| u |y| <= u |y| for
                    |slope| <= 0.5 - which is why the slopes here stay inside it (the network's are 0.1 .. 0.4)
  depthwise 3x3     12 u (|scale| m + |shift|): nine fused multiply-adds (9 u m), then the same affine and PReLU
  average pool      10 u sum |x| / 9: eight additions and the division;   max pool, preprocess, argmax, counts: exact
  channel scale     2 ulp of the result
  PMCA weights      the kernel's chain of float32 operations up to the sigmoid is restated in its own order (pmca_chain32: correctly
                    rounded float32 fused multiply-adds, sequential), so summation order drops out; the sigmoid of that value is held to
                    the rule for expf below.  The restated chain itself is held to the float64 oracle by its forward bound (pmca_bound)
  MAD gate          expf has no bound written into the kernel: max error <= 2 x that of float32 torch on the same input + 1 ulp"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import lmffnet_torch as L
from quber_amd import _lib

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TRIP = 4096 * 256          # work items of one trip of a grid_for launch


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_ALIVE = []


def dev(a):
    """upload; the tensor lives until the end of the test (a launch takes raw addresses: nothing else holds its operands)"""
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return _ALIVE[-1]


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class View:
    """Channels c0 .. c0 + C of frames 0 .. B - 1 of a NaN-filled float32 buffer [B + 1][H][W][cs]; `data` [B,H,W,C] makes it a source."""

    def __init__(self, B, H, W, cs, c0, C_, data=None):
        self.B, self.c0, self.C, self.cs = B, c0, C_, cs
        self.host = np.full((B + 1, H, W, cs), np.nan, np.float32)
        if data is not None:
            self.host[:B, :, :, c0:c0 + C_] = data
        self.dev = dev(self.host)

    @property
    def p(self):
        return ptr(self.dev, 4 * self.c0)

    def fetch(self):
        """the view after the launch, NCHW float64; asserts that every byte outside it is unchanged"""
        torch.cuda.synchronize()
        a = self.dev.cpu().numpy()
        outside = np.ones(a.shape, bool)
        outside[:self.B, :, :, self.c0:self.c0 + self.C] = False
        assert np.array_equal(bits(a)[outside], bits(self.host)[outside]), "bytes outside the destination slice were written"
        return torch.from_numpy(a[:self.B, :, :, self.c0:self.c0 + self.C].copy()).double().permute(0, 3, 1, 2)

    def untouched(self):
        torch.cuda.synchronize()
        return np.array_equal(bits(self.dev.cpu().numpy()), bits(self.host))


def nchw(a):
    return torch.from_numpy(a).double().permute(0, 3, 1, 2)


def per_channel(rng, C_):
    """distinct scale / shift / slope per channel; slopes of both signs"""
    scale = rng.uniform(0.5, 1.5, C_).astype(np.float32) * rng.choice([-1, 1], C_).astype(np.float32)
    shift = rng.normal(0, 0.3, C_).astype(np.float32)
    slope = np.linspace(-0.5, 0.5, C_).astype(np.float32)[rng.permutation(C_)]
    return scale, shift, slope


def prelu_affine(t, scale, shift, slope):
    e = lambda a: torch.from_numpy(a).double()[None, :, None, None]
    y = t * e(scale) + e(shift)
    return torch.where(y > 0, y, y * e(slope)), e(scale).abs(), e(shift).abs()


def within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                       # a NaN is outside every bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"{what}: max error {float(err.max()):.3e}, {ratio:.3f} of the bound")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound, worst {ratio:.2f}x"


def refused(rc, text):
    assert rc != 0
    assert text in _lib.load().quber_last_error().decode()


# ---- preprocess ----
@pytest.mark.parametrize("h,w", [(1, 1), (7, 9), (1024, 1025)], ids=["1px", "63px", "second-trip"])
def test_preprocess(h, w):
    rng = np.random.default_rng(h * w)
    bgr = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    dep = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    bgr[0, 0], dep[0, 0] = (0, 255, 128), (255, 0, 1)
    assert (h * w > TRIP) == (h == 1024)
    x = dev(np.full((h * w + 1, 8), np.nan, np.float32))
    assert _lib.load().quber_op_lmff_preprocess(ptr(dev(bgr)), ptr(dev(dep)), h * w, ptr(x), stream()) == 0
    torch.cuda.synchronize()
    got = x.cpu().numpy()
    ref = L.preprocess(bgr, dep)[0].permute(1, 2, 0).reshape(h * w, 6).numpy()
    assert np.array_equal(bits(got[:-1, :6]), bits(ref))
    assert (bits(got[:-1, 6:]) == 0).all() and np.isnan(got[-1]).all()


# ---- depthwise 3x3 + BN + PReLU ----
DW_VIEWS = {"16@16of32-four-wide": (32, 16, 16), "262of264-one-wide": (264, 0, 262), "48@2of52-misaligned": (52, 2, 48)}


def run_dwconv(B, H, W, cs, c0, C_, dil, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, C_)).astype(np.float32)
    w9 = rng.normal(0, 0.4, (C_, 3, 3)).astype(np.float32)
    scale, shift, slope = per_channel(rng, C_)
    src, dst = View(B, H, W, cs, c0, C_, x), View(B, H, W, cs, c0, C_)
    rc = _lib.load().quber_op_lmff_dwconv(src.p, cs, dst.p, cs, B, H, W, C_, dil, ptr(dev(w9)), ptr(dev(scale)), ptr(dev(shift)),
                                          ptr(dev(slope)), stream())
    assert rc == 0, _lib.load().quber_last_error()
    xp, wt = F.pad(nchw(x), (dil, dil, dil, dil)), torch.from_numpy(w9).double()
    acc, mag = 0.0, 0.0                                    # the nine taps as shifted products: sum x w and sum |x w|
    for ky in range(3):
        for kx in range(3):
            t = xp[:, :, ky * dil:ky * dil + H, kx * dil:kx * dil + W] * wt[None, :, ky, kx, None, None]
            acc, mag = acc + t, mag + t.abs()
    ref, s, sh = prelu_affine(acc, scale, shift, slope)
    within(dst.fetch(), ref, 12 * U * (s * mag + sh), f"dwconv {B}x{H}x{W}x{C_} dil {dil}")


@pytest.mark.parametrize("view", DW_VIEWS, ids=list(DW_VIEWS))
@pytest.mark.parametrize("dil", [1, 2, 32])
@pytest.mark.parametrize("h,w", [(9, 13), (8, 12)])
def test_dwconv(h, w, dil, view):
    """batch 2; dilation 32 on these maps: only the centre tap meets the map"""
    run_dwconv(2, h, w, *DW_VIEWS[view], dil, seed=h * 100 + dil)


def test_dwconv_single_pixel():
    for view in DW_VIEWS.values():
        run_dwconv(2, 1, 1, *view, 1, seed=5)


@pytest.mark.parametrize("h,w,cs,c", [(64, 64, 132, 130), (128, 128, 132, 132)], ids=["one-wide", "four-wide"])
def test_dwconv_second_grid_stride_trip(h, w, cs, c):
    """more work items than one trip of the grid covers: 2 x 64 x 64 x 130 one-wide, 2 x 128 x 128 x 132 / 4 four-wide"""
    assert 2 * h * w * c // (4 if c % 4 == 0 else 1) > TRIP
    run_dwconv(2, h, w, cs, 0, c, 2, seed=c)


def test_dwconv_refuses_2_31_elements():
    d = dev(np.zeros(64, np.float32))
    rc = _lib.load().quber_op_lmff_dwconv(ptr(d), 1, ptr(d), 1, 32768, 256, 256, 1, 1, ptr(d), ptr(d), ptr(d), ptr(d), stream())
    refused(rc, "dwconv: tensor too large")


# ---- pooling ----
def run_pool(B, H, W, in_cs, in_c0, C_, out_cs, out_c0, mode, OH, OW, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, C_)).astype(np.float32)
    src, dst = View(B, H, W, in_cs, in_c0, C_, x), View(B, OH, OW, out_cs, out_c0, C_)
    rc = _lib.load().quber_op_lmff_pool(src.p, in_cs, dst.p, out_cs, B, H, W, C_, OH, OW, mode, stream())
    assert rc == 0, _lib.load().quber_last_error()
    got = dst.fetch()
    if mode == 1:
        assert torch.equal(got, F.max_pool2d(nchw(x), 2, 2))
    else:
        within(got, F.avg_pool2d(nchw(x), 3, 2, 1), 10 * U * F.avg_pool2d(nchw(x).abs(), 3, 2, 1), f"avg pool {H}x{W}x{C_}")


@pytest.mark.parametrize("dst", [(40, 32), (136, 128), (264, 256)], ids=["32of40", "128of136", "256of264"])
@pytest.mark.parametrize("h,w", [(9, 13), (8, 12)])
def test_avgpool_injection_slices(h, w, dst):
    """the six input channels (cs 8) into the tail of each concatenation buffer, one channel per lane; odd and even maps"""
    run_pool(2, h, w, 8, 0, 6, dst[0], dst[1], 0, (h + 1) // 2, (w + 1) // 2, seed=h + dst[0])


@pytest.mark.parametrize("h,w", [(9, 13), (8, 12)])
def test_avgpool_four_wide(h, w):
    run_pool(2, h, w, 40, 0, 40, 48, 4, 0, (h + 1) // 2, (w + 1) // 2, seed=h)


@pytest.mark.parametrize("h,w", [(8, 12), (9, 13)])
def test_maxpool_38_of_40_into_26_of_64(h, w):
    """exact; the odd map drops its last row and column like MaxPool2d(2, 2)"""
    run_pool(2, h, w, 40, 0, 38, 64, 26, 1, h // 2, w // 2, seed=h)


def test_maxpool_four_wide():
    run_pool(2, 8, 12, 40, 0, 40, 64, 24, 1, 4, 6, seed=3)


@pytest.mark.parametrize("mode,h,c,cs", [(0, 592, 6, 8), (1, 460, 40, 40)], ids=["avg-one-wide", "max-four-wide"])
def test_pool_second_grid_stride_trip(mode, h, c, cs):
    assert 2 * (h // 2) ** 2 * c // (4 if c % 4 == 0 else 1) > TRIP
    run_pool(2, h, h, cs, 0, c, cs, 0, mode, h // 2, h // 2, seed=h)


def test_maxpool_window_outside_the_map_is_refused():
    """a 9-row map has four full 2 x 2 windows per column: five output rows are refused by the launcher, nothing is launched"""
    x = np.random.default_rng(0).standard_normal((2, 9, 12, 40)).astype(np.float32)
    src, dst = View(2, 9, 12, 40, 0, 38, x[..., :38]), View(2, 5, 6, 64, 26, 38)
    refused(_lib.load().quber_op_lmff_pool(src.p, 40, dst.p, 64, 2, 9, 12, 38, 5, 6, 1, stream()), "max pool window leaves the map")
    refused(_lib.load().quber_op_lmff_pool(src.p, 40, dst.p, 64, 2, 9, 12, 38, 4, 7, 1, stream()), "max pool window leaves the map")
    assert dst.untouched()


def test_pool_refuses_2_31_elements():
    d = dev(np.zeros(64, np.float32))
    refused(_lib.load().quber_op_lmff_pool(ptr(d), 1, ptr(d), 1, 32768, 512, 512, 1, 256, 256, 0, stream()), "pool: tensor too large")


# ---- BN + PReLU of a tensor or of a sum ----
def run_affine(B, H, W, a_cs, C_, b_cs, out_cs, out_c0, seed):
    """b_cs 0: no addend"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, H, W, C_)).astype(np.float32)
    b = rng.standard_normal((B, H, W, C_)).astype(np.float32)
    a[0, 0, :, :] = 0                                      # exact zeros: y = shift, and its sign decides
    b[0, 0, :, :] = 0
    a[0, -1] = -np.abs(a[0, -1])
    b[0, -1, 0] = -a[0, -1, 0]                             # a + b = 0 exactly
    scale, shift, slope = per_channel(rng, C_)
    shift[::5] = 0                                         # ... and y = 0 exactly: not positive
    sa, sb, dst = View(B, H, W, a_cs, 0, C_, a), (View(B, H, W, b_cs, 0, C_, b) if b_cs else None), View(B, H, W, out_cs, out_c0, C_)
    rc = _lib.load().quber_op_lmff_affine(sa.p, a_cs, sb.p if sb else None, b_cs, dst.p, out_cs, B, H, W, C_, ptr(dev(scale)), ptr(dev(shift)),
                                          ptr(dev(slope)), stream())
    assert rc == 0, _lib.load().quber_last_error()
    t = nchw(a) + nchw(b) if b_cs else nchw(a)
    mag = nchw(a).abs() + (nchw(b).abs() if b_cs else 0)
    ref, s, sh = prelu_affine(t, scale, shift, slope)
    within(dst.fetch(), ref, 3 * U * mag * s + U * sh, f"affine {C_} of {a_cs}, addend cs {b_cs}")


@pytest.mark.parametrize("addend", [False, True], ids=["plain", "sum"])
@pytest.mark.parametrize("c,cs", [(38, 40), (64, 64), (134, 136), (262, 264)])
def test_affine(c, cs, addend):
    """the channel counts of the plan: 64 is the four-wide form, the sliced ones take one channel per lane"""
    run_affine(2, 5, 7, cs, c, cs if addend else 0, cs, 0, seed=c)


def test_affine_addend_at_another_stride_and_sliced_destination():
    run_affine(2, 5, 7, 64, 64, 136, 136, 64, seed=1)      # four-wide: SEM_B's output into a slice of the concatenation buffer
    run_affine(2, 5, 7, 40, 38, 64, 40, 0, seed=2)


@pytest.mark.parametrize("c,cs,h,w", [(38, 40, 120, 116), (64, 64, 182, 182)], ids=["one-wide", "four-wide"])
def test_affine_second_grid_stride_trip(c, cs, h, w):
    assert 2 * h * w * c // (4 if c % 4 == 0 else 1) > TRIP
    run_affine(2, h, w, cs, c, cs, cs, 0, seed=c)


def test_affine_refuses_2_31_elements():
    d = dev(np.zeros(64, np.float32))
    refused(_lib.load().quber_op_lmff_affine(ptr(d), 1, None, 0, ptr(d), 1, 32768, 256, 256, 1, ptr(d), ptr(d), ptr(d), stream()),
            "affine: tensor too large")


# ---- PMCA channel weights ----
def pmca_params(rng, C_):
    return {"p.conv2x2.conv.weight": rng.normal(0, 0.5, (C_, 1, 2, 2)).astype(np.float32),
            "p.SE_Block.fc.0.weight": rng.normal(0, C_ ** -0.5, (C_ // 8, C_)).astype(np.float32),
            "p.SE_Block.fc.1.weight": np.array([0.3], np.float32),
            "p.SE_Block.fc.2.weight": rng.normal(0, 1.0, (C_, C_ // 8)).astype(np.float32)}


def pmca_bound(x, w):
    """Forward error bound of the PMCA weights per element [B,C], in float64, for the kernel's arithmetic: bin and global averages from
    float64 sums rounded to float32, s = four fused multiply-adds + the global average (6 u (sum |p w| + |mean|)), the two fully connected
    layers as sequential chains of n fused multiply-adds (n u sum |v w| plus the error carried in), the PReLU's product (u |h|), and the
    sigmoid: slope at most 1/4, expf to 1 ulp (the accuracy the HIP math library documents for it), the addition and the correctly
    rounded division - 4 u."""
    C_ = x.shape[1]
    w2, fc0, alpha, fc2 = (torch.from_numpy(w["p." + k]).double() for k in ("conv2x2.conv.weight", "SE_Block.fc.0.weight", "SE_Block.fc.1.weight",
                                                                              "SE_Block.fc.2.weight"))
    pooled, mean = F.adaptive_avg_pool2d(x, (2, 2)), F.adaptive_avg_pool2d(x, 1).flatten(1)
    s = (pooled * w2[None, :, 0]).sum((2, 3)) + mean
    ds = 6 * U * ((pooled.abs() * w2[None, :, 0].abs()).sum((2, 3)) + mean.abs())
    h = s @ fc0.T
    dh = C_ * U * (s.abs() @ fc0.abs().T) + ds @ fc0.abs().T + U * h.abs()
    hid = torch.where(h > 0, h, h * alpha)
    do = (C_ // 8) * U * (hid.abs() @ fc2.abs().T) + dh @ fc2.abs().T
    return 0.25 * do + 4 * U


def fma32(a, b, c):
    """float32 fma(a, b, c), correctly rounded.  The product of two float32 is exact in float64; the float64 sum is rounded to odd (TwoSum
    gives its error: when it is inexact, of the two float64 neighbours of the exact sum the one with an odd last bit is taken); rounding
    that to float32 is then the single rounding of the exact result."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def pmca_chain32(bins, mean, w):
    """pmca_fc_kernel up to the sigmoid, operation by operation in float32: bins [B,C,4] / mean [B,C] = the float64 bin and global averages.
    -> the pre-sigmoid value o [B,C] float32"""
    f = np.float32
    w2, fc0, alpha, fc2 = (w["p." + k] for k in ("conv2x2.conv.weight", "SE_Block.fc.0.weight", "SE_Block.fc.1.weight", "SE_Block.fc.2.weight"))
    B, C_ = mean.shape
    w2, p = w2.reshape(C_, 4), bins.astype(f)
    o1 = np.zeros((B, C_), f)
    for k in range(4):
        o1 = fma32(p[:, :, k], w2[None, :, k], o1)
    s = o1 + mean.astype(f)
    h = np.zeros((B, C_ // 8), f)
    for k in range(C_):
        h = fma32(s[:, k:k + 1], fc0[None, :, k], h)
    hid = np.where(h > 0, h, h * alpha[0])
    o = np.zeros((B, C_), f)
    for k in range(C_ // 8):
        o = fma32(hid[:, k:k + 1], fc2[None, :, k], o)
    assert s.dtype == f and hid.dtype == f and o.dtype == f
    return o


def adaptive_bins(x):
    """float64 averages of the 2 x 2 adaptive bins [0, ceil(n/2)) and [floor(n/2), n) per axis, and of the whole map: x [B,H,W,C]"""
    B, H, W, C_ = x.shape
    x = x.astype(np.float64)
    ys, xs = ((0, (H + 1) // 2), (H // 2, H)), ((0, (W + 1) // 2), (W // 2, W))
    bins = np.stack([x[:, y0:y1, x0:x1].mean((1, 2)) for y0, y1 in ys for x0, x1 in xs], 2)
    return bins, x.mean((1, 2))


def check_sigmoid(wts, o, ref64, bound64, what):
    """wts: the kernel's weights; o: the restated chain's pre-sigmoid value.  The expf rule on the sigmoid alone: the kernel is no further
    from the float64 sigmoid of o than twice float32 torch's sigmoid of the same o, plus 1 ulp.  And the restated chain is the operation:
    its sigmoid is within the chain's forward bound of the float64 oracle ref64."""
    o = torch.from_numpy(o)
    sig64, sig32 = torch.sigmoid(o.double()), torch.sigmoid(o).double()
    within(sig64, ref64, bound64, what + " (restated chain against the float64 oracle)")
    got = torch.from_numpy(wts).double()
    e_hip, e_t32 = float((got - sig64).abs().max()), float((sig32 - sig64).abs().max())
    ulp = float(np.spacing(np.float32(sig64.abs().max())))
    print(f"{what}: HIP {e_hip:.3e}, float32 torch {e_t32:.3e}, 1 ulp {ulp:.3e}; against the float64 oracle {float((got - ref64).abs().max()):.3e}")
    assert e_hip <= 2 * e_t32 + ulp, f"{what}: HIP {e_hip:.3e}, float32 torch {e_t32:.3e}, 1 ulp {ulp:.3e}"


def launch_pmca(src, B, H, W, C_, w, wts=None):
    lib = _lib.load()
    sums = dev(np.full((B + 1) * C_ * 5, np.nan, np.float64))
    wts = dev(np.full((B + 1, C_), np.nan, np.float32)) if wts is None else wts
    rc = lib.quber_op_lmff_pmca(src.p, src.cs, B, H, W, C_, ptr(dev(w["p.conv2x2.conv.weight"])), ptr(dev(w["p.SE_Block.fc.0.weight"])),
                                ptr(dev(w["p.SE_Block.fc.1.weight"])), ptr(dev(w["p.SE_Block.fc.2.weight"])), ptr(wts), ptr(sums), stream())
    torch.cuda.synchronize()
    return rc, wts.cpu().numpy(), sums.cpu().numpy().reshape(B + 1, C_ * 5)


def check_pmca(x, C_, cs, c0, seed):
    B, H, W = x.shape[:3]
    w = pmca_params(np.random.default_rng(seed), C_)
    rc, wts, sums = launch_pmca(View(B, H, W, cs, c0, C_, x), B, H, W, C_, w)
    assert rc == 0, _lib.load().quber_last_error()
    assert np.isnan(wts[B]).all() and np.isnan(sums[B]).all(), "the frame behind the batch was written"
    with torch.no_grad():
        ref = L.pmca_weights(nchw(x), {k: torch.from_numpy(v).double() for k, v in w.items()}, "p")
    check_sigmoid(wts[:B], pmca_chain32(*adaptive_bins(x), w), ref, pmca_bound(nchw(x), w), f"pmca {B}x{H}x{W}x{C_}")


@pytest.mark.parametrize("c,cs,c0", [(64, 64, 0), (128, 136, 4)], ids=["64", "128@4of136"])
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (9, 11), (15, 20)])
def test_pmca(h, w, c, cs, c0):
    """batch 3, three different frames; odd sizes: the two bins of an axis share the middle row / column"""
    x = np.random.default_rng(h * w + c).standard_normal((3, h, w, c)).astype(np.float32) + np.float32(0.5)
    check_pmca(x, c, cs, c0, seed=h + c)


def test_pmca_two_rows_per_block_and_a_short_last_band():
    """345 x 3 rows > 1024: every block takes two rows and the last band holds one"""
    x = np.random.default_rng(7).standard_normal((3, 345, 4, 64)).astype(np.float32) + np.float32(0.25)
    check_pmca(x, 64, 64, 0, seed=7)


@pytest.mark.parametrize("h,w", [(4, 6), (9, 11), (5, 4)])
@pytest.mark.parametrize("c", [64, 128])
def test_pmca_closed_form(h, w, c):
    """An input that is constant per (frame, channel, quadrant): every 2 x 2 bin average and the global average are known without summing.
    Even map: four different quadrant values v_k, bins = v_k, global = their area-weighted mean; odd map: one value v, every bin = v
    whatever its overlap - a wrong divisor or bin edge changes it.  Values are small integers / 8: sums are exact in any order."""
    rng = np.random.default_rng(h * w + c)
    B = 3
    v = rng.integers(-16, 17, (B, 2, 2, c)).astype(np.float64) / 8
    if h % 2 or w % 2:
        v[:] = v[:, :1, :1]
    x = np.zeros((B, h, w, c), np.float32)
    hy, hx = (h + 1) // 2, (w + 1) // 2
    x[:, :hy, :hx], x[:, :hy, hx:], x[:, hy:, :hx], x[:, hy:, hx:] = v[:, :1, :1], v[:, :1, 1:], v[:, 1:, :1], v[:, 1:, 1:]
    area = np.array([[hy * hx, hy * (w - hx)], [(h - hy) * hx, (h - hy) * (w - hx)]], np.float64)[None, :, :, None]
    glob = (v * area).sum((1, 2)) / (h * w)                                   # [B,c]
    w_ = pmca_params(np.random.default_rng(c), c)
    w64 = {k: a.astype(np.float64) for k, a in w_.items()}
    s = (v.transpose(0, 3, 1, 2).reshape(B, c, 4) * w64["p.conv2x2.conv.weight"].reshape(c, 4)).sum(2) + glob
    hid = s @ w64["p.SE_Block.fc.0.weight"].T
    hid = np.where(hid > 0, hid, hid * np.float64(w_["p.SE_Block.fc.1.weight"][0]))
    ref = 1 / (1 + np.exp(-(hid @ w64["p.SE_Block.fc.2.weight"].T)))
    rc, wts, _ = launch_pmca(View(B, h, w, c, 0, c, x), B, h, w, c, w_)
    assert rc == 0
    o = pmca_chain32(v.transpose(0, 3, 1, 2).reshape(B, c, 4), glob, w_)      # the chain on the known averages: nothing is summed
    check_sigmoid(wts[:B], o, torch.from_numpy(ref), pmca_bound(nchw(x), w_), f"pmca closed form {h}x{w}x{c}")


def test_pmca_refuses_other_channel_counts_and_misaligned_views():
    x = np.ones((2, 4, 4, 64), np.float32)
    wts = dev(np.full((3, 64), np.nan, np.float32))
    for c in (32, 96):
        rc, got, _ = launch_pmca(View(2, 4, 4, 64, 0, 64, x), 2, 4, 4, c, pmca_params(np.random.default_rng(0), 64), wts)
        refused(rc, "pmca: expects 64 or 128 channels")
    rc, got, _ = launch_pmca(View(2, 4, 4, 72, 2, 64, x), 2, 4, 4, 64, pmca_params(np.random.default_rng(0), 64), wts)     # base 8 bytes off
    refused(rc, "pmca: channels must come in aligned groups of 4")
    rc, got, _ = launch_pmca(View(2, 4, 4, 66, 0, 64, x), 2, 4, 4, 64, pmca_params(np.random.default_rng(0), 64), wts)     # cs no multiple of 4
    refused(rc, "pmca: channels must come in aligned groups of 4")
    assert np.isnan(got).all()


# ---- channel scale, MAD gate ----
@pytest.mark.parametrize("h,w,c,cs,out_cs,out_c0", [(17, 19, 3, 4, 4, 0), (9, 11, 64, 64, 136, 64), (9, 11, 128, 128, 264, 128), (420, 420, 3, 4, 4, 0)],
                         ids=["3of4", "64-into-64of136", "128-into-128of264", "second-trip"])
def test_scale_channels(h, w, c, cs, out_cs, out_c0):
    B = 2
    assert (B * h * w * c > TRIP) == (h == 420) and (h * w) % 256
    rng = np.random.default_rng(h + c)
    x = rng.standard_normal((B, h, w, c)).astype(np.float32)
    wts = rng.uniform(0.05, 0.95, (B, c)).astype(np.float32)
    src, dst = View(B, h, w, cs, 0, c, x), View(B, h, w, out_cs, out_c0, c)
    assert _lib.load().quber_op_lmff_scale(src.p, cs, ptr(dev(wts)), dst.p, out_cs, B, h, w, c, stream()) == 0
    ref = L.channel_scale(nchw(x), torch.from_numpy(wts).double())
    within(dst.fetch(), ref, 2 * torch.from_numpy(np.spacing(ref.abs().float().numpy())).double(), f"scale {h}x{w}x{c}")


@pytest.mark.parametrize("h,w", [(17, 19), (420, 420)], ids=["small", "second-trip"])
def test_mad_gate(h, w):
    """C = 3 of cs 4, NHWC in, planar out, batch 2, h * w no multiple of 256"""
    B, c = 2, 3
    assert (B * h * w * c > TRIP) == (h == 420) and (h * w) % 256
    rng = np.random.default_rng(h)
    o = rng.standard_normal((B, h, w, c)).astype(np.float32)
    att = (rng.standard_normal((B, h, w, c)) * 4).astype(np.float32)
    att[0, 0, :3] = [[0, 0, 0], [-100, 100, -20], [20, -0.0, 1e-8]]
    so, sa = View(B, h, w, 4, 0, c, o), View(B, h, w, 4, 0, c, att)
    q = dev(np.full((B + 1, c, h * w), np.nan, np.float32))
    assert _lib.load().quber_op_lmff_gate(so.p, 4, sa.p, 4, ptr(q), B, h, w, c, stream()) == 0
    torch.cuda.synchronize()
    got = q.cpu().numpy()
    assert np.isnan(got[B]).all()
    got = torch.from_numpy(got[:B]).double().reshape(B, c, h, w)
    ref = L.mad_gate(nchw(o), nchw(att))
    t32 = L.mad_gate(nchw(o).float(), nchw(att).float()).double()
    e_hip, e_t32 = float((got - ref).abs().max()), float((t32 - ref).abs().max())
    ulp = float(np.spacing(np.float32(ref.abs().max())))
    print(f"gate {h}x{w}: HIP {e_hip:.3e}, float32 torch {e_t32:.3e}, 1 ulp {ulp:.3e}")
    assert e_hip <= 2 * e_t32 + ulp


# ---- foreground filter: argmax + overlap counts ----
def run_filter(B, nc, cls, hw, K, seed, ties=False):
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((B, nc, hw)).astype(np.float32)
    if ties:
        lg = np.round(lg)                                   # many exact ties between planes, the maximum included
    masks = rng.choice(np.array([0, 0, 1, 128, 255], np.uint8), (B, max(K, 1), hw))
    if K > 1:
        masks[:, 1] = 0                                     # an empty mask: its counts stay 0
    fg = dev(np.full((B + 1, hw), 7, np.uint8))
    counts = dev(np.full((B + 1, max(K, 1), 2), -1, np.int64))
    rc = _lib.load().quber_foreground_filter(ptr(dev(lg)), nc, cls, ptr(dev(masks)) if K else None, B, K, hw, ptr(fg), ptr(counts), stream())
    assert rc == 0, _lib.load().quber_last_error()
    torch.cuda.synchronize()
    fg, counts = fg.cpu().numpy(), counts.cpu().numpy()
    exp = (np.argmax(lg, axis=1) == cls)                    # numpy: the first maximum wins
    assert np.array_equal(fg[:B], exp.astype(np.uint8)) and (fg[B] == 7).all()
    assert (counts[B] == -1).all()
    if K:
        on = masks != 0
        assert np.array_equal(counts[:B, :, 0], (on & exp[:, None]).sum(2)) and np.array_equal(counts[:B, :, 1], on.sum(2))
    else:
        assert (counts == -1).all()
    return lg, fg


@pytest.mark.parametrize("hw", [1, 63, 256 * 16 + 1])
@pytest.mark.parametrize("K", [1, 37])
def test_foreground_filter_counts(hw, K):
    """batch 2, masks holding 1, 128 and 255, one all-zero mask; hw one past what a block column covers"""
    run_filter(2, 3, 2, hw, K, seed=hw + K)


@pytest.mark.parametrize("nc,cls", [(3, 2), (3, 0), (3, 1), (2, 0), (2, 1), (5, 3)])
def test_foreground_filter_ties_and_classes(nc, cls):
    lg, fg = run_filter(2, nc, cls, 4097, 3, seed=nc * 10 + cls, ties=True)
    top = lg.max(1)
    tie = (lg[:, 0] == top) & (lg[:, nc - 1] == top)
    assert tie.any()
    if cls == nc - 1 and nc > 1:
        assert (fg[:2][tie] == 0).all()                    # class 0 ties the last class: the first maximum wins


def test_foreground_filter_without_masks_and_second_trip():
    run_filter(2, 3, 2, 100, 0, seed=1)
    assert 2 * (256 * 16 * 130 + 1) > TRIP
    run_filter(2, 3, 2, 256 * 16 * 130 + 1, 1, seed=2)


def test_foreground_filter_refuses_mask_counts_outside_the_grid():
    """a negative count would reach the clearing launch as a huge size, a count above 65535 is no grid dimension: both are refused on the
    host, before anything is launched"""
    lg = dev(np.zeros((1, 3, 16), np.float32))
    fg = dev(np.full(16, 7, np.uint8))
    counts = dev(np.full(8, -1, np.int64))
    masks = dev(np.ones(16, np.uint8))
    for k in (-1, 65536):
        refused(_lib.load().quber_foreground_filter(ptr(lg), 3, 2, ptr(masks), 1, k, 16, ptr(fg), ptr(counts), stream()), "n_masks outside 0..65535")
    torch.cuda.synchronize()
    assert (fg.cpu().numpy() == 7).all() and (counts.cpu().numpy() == -1).all()
