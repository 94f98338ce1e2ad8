"""CPU: the float64 restatements of the glue operations (oracle/glue_np.py) against torch.nn.functional in float64, on odd sizes
and a 1x1 source.  tests/test_gpu_glue.py holds the HIP kernels against these references."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import glue_np as G


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def nhwc(t):
    return np.transpose(t.numpy(), (0, 2, 3, 1))


@pytest.mark.parametrize("shape,groups", [((2, 7, 9, 32), 32), ((1, 1, 1, 64), 32), ((3, 5, 3, 320), 32), ((1, 3, 5, 2048), 32), ((2, 4, 4, 12), 3)])
@pytest.mark.parametrize("relu", [False, True])
def test_group_norm(shape, groups, relu):
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) * 3 + 1).astype(np.float32)
    gam = (rng.random(shape[3]) + 0.5).astype(np.float32)
    bet = rng.standard_normal(shape[3]).astype(np.float32)
    ref = F.group_norm(nchw(x).double(), groups, torch.from_numpy(gam).double(), torch.from_numpy(bet).double(), 1e-5)
    ref = ref.relu() if relu else ref
    got = G.group_norm(x, groups, gam, bet, 1e-5, relu)
    assert got.dtype == np.float64
    # float64 on both sides: two orders of the same few operations
    np.testing.assert_allclose(got, nhwc(ref), rtol=1e-12, atol=1e-12)
    sums = G.group_sums(x, groups)
    n = shape[1] * shape[2] * (shape[3] // groups)
    xg = x.astype(np.float64).reshape(shape[0], -1, groups, shape[3] // groups)
    np.testing.assert_allclose(sums[..., 0] / n, xg.mean(axis=(1, 3)), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(sums[..., 1] / n, (xg * xg).mean(axis=(1, 3)), rtol=1e-13)


def test_group_norm_f32_form_is_a_float32_implementation():
    """The float32 restatement of torch's CPU form is as far from float64 as torch's own float32 kernel: both lose ~ulp(|x * scale|)
    per operation (x ~ 100, scale ~ 1: ulp 7.6e-6, three roundings), nowhere near the 2e-6 bar of the randn * 3 + 1 inputs."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 9, 11, 64)) + 100).astype(np.float32)
    gam = (rng.random(64) + 0.5).astype(np.float32)
    bet = rng.standard_normal(64).astype(np.float32)
    ref = G.group_norm(x, 32, gam, bet)
    own = G.group_norm(x, 32, gam, bet, torch_f32_form=True)
    tor = nhwc(F.group_norm(nchw(x), 32, torch.from_numpy(gam), torch.from_numpy(bet), 1e-5))
    assert own.dtype == np.float32
    e_own, e_tor = np.abs(own - ref).max(), np.abs(tor - ref).max()
    print(f"offset input: float32 form {e_own:.2e}, torch float32 {e_tor:.2e} from float64")
    assert 2e-6 < e_own < 5e-5 and 2e-6 < e_tor < 5e-5


@pytest.mark.parametrize("shape", [(2, 7, 9, 4), (1, 8, 6, 8), (1, 1, 9, 4), (2, 7, 1, 4), (1, 1, 1, 4), (1, 11, 15, 12)])
def test_maxpool(shape):
    rng = np.random.default_rng(sum(shape))
    x = (-1 - rng.random(shape)).astype(np.float32)          # all negative: a zero padding would show
    ref = F.max_pool2d(nchw(x).double(), 3, 2, 1)
    got = G.maxpool3x3s2(x)
    assert got.dtype == x.dtype
    np.testing.assert_array_equal(got.astype(np.float64), nhwc(ref))


@pytest.mark.parametrize("shape,out", [((1, 1, 1, 4), (30, 40)), ((2, 5, 7, 4), (10, 14)), ((1, 5, 7, 8), (20, 28)), ((1, 7, 9, 4), (10, 31)),
                                       ((2, 6, 5, 4), (6, 5)), ((1, 9, 7, 4), (4, 3))])
def test_bilinear(shape, out):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    got = G.bilinear(x, *out)
    assert got.dtype == np.float64
    # torch's float32 path: the same coordinates and weights, the blend rounded to float32 at every step - three weighted sums of
    # values up to max|x|: a few ulp of max|x|.  Its `scale * (dst + 0.5) - 0.5` is one fma or two operations depending on how the
    # host code was compiled (7x9 -> 10x31, column 15: 4.0 against 3.9999998, measured): every element agrees with one of the two
    f32 = nhwc(F.interpolate(nchw(x), size=out, mode="bilinear", align_corners=False))
    near = np.minimum(np.abs(got - f32), np.abs(G.bilinear(x, *out, fused_coords=True) - f32))
    assert near.max() <= 4 * 2.0 ** -24 * np.abs(x).max()
    # the float64 path differs only through its float64 coordinates: equal where the ratio and every coordinate are exact in float32
    if all(i == 1 or (o % i == 0 and (o // i) & (o // i - 1) == 0) for i, o in zip(shape[1:3], out)):
        f64 = nhwc(F.interpolate(nchw(x).double(), size=out, mode="bilinear", align_corners=False))
        np.testing.assert_allclose(got, f64, rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("h,w,OH,OW", [(14, 19, 53, 75), (3, 4, 12, 16), (1, 1, 4, 4), (5, 3, 17, 12)])
def test_upsample_logits(h, w, OH, OW):
    rng = np.random.default_rng(h * w)
    q = rng.standard_normal((2, 6, h, w)).astype(np.float32)
    got = G.upsample_logits(q, 4, OH, OW, 0xC)
    full = F.interpolate(torch.from_numpy(q).double(), scale_factor=4, mode="bilinear", align_corners=False).numpy()[:, :, :OH, :OW]
    full[:, 2:4] *= 4                            # (x4: every coordinate k / 4 + 1 / 8 - 1 / 2 is exact in float32)
    np.testing.assert_allclose(got, full, rtol=1e-14, atol=1e-14)
    np.testing.assert_array_equal(G.upsample_logits(q, 4, OH, OW, 0)[:, 2:4] * 4, got[:, 2:4])
    with pytest.raises(AssertionError):
        G.upsample_logits(q, 4, 4 * h + 1, OW)


@pytest.mark.parametrize("shape", [(2, 1, 1, 4), (1, 3, 5, 68), (2, 13, 23, 8)])
def test_avgpool(shape):
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) + 2).astype(np.float32)
    ref = F.adaptive_avg_pool2d(nchw(x).double(), 1).numpy()[:, :, 0, 0]
    np.testing.assert_allclose(G.avgpool(x), ref, rtol=1e-13)


@pytest.mark.parametrize("C,cout", [(32, 1), (32, 3), (64, 4), (64, 2)])
def test_predictor_and_activations(C, cout):
    rng = np.random.default_rng(C + cout)
    x = rng.standard_normal((2, 5, 7, C)).astype(np.float32)
    w = (rng.standard_normal((cout, C)) * 0.3).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    z = G.predictor_logits(x, w, b)
    ref = F.conv2d(nchw(x).double(), torch.from_numpy(w).double()[:, :, None, None], torch.from_numpy(b).double())
    np.testing.assert_allclose(z, ref.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(G.softmax(z, 1), torch.softmax(ref, 1).numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(G.sigmoid(z), torch.sigmoid(ref).numpy(), rtol=1e-13, atol=1e-15)


def test_preprocess_add_copy():
    rng = np.random.default_rng(3)
    B, H, W = 2, 5, 7
    bgr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    dep = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    offs = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    mean, std = [103.53, 116.28, 123.675, 127.5, 127.5, 127.5], [1.0, 57.375, 58.395, 2.0, 127.5, 3.0]
    x = G.preprocess(bgr, dep, offs, mean, std, xc=16)
    assert x.shape == (2, B, H, W, 16) and not x[..., 6:].any()
    np.testing.assert_array_equal(x[0, ..., :3], (bgr.astype(np.float64) - np.array(mean[:3])) / np.array(std[:3]))
    np.testing.assert_array_equal(x[1, ..., :3], (dep.astype(np.float64) - np.array(mean[3:])) / np.array(std[3:]))
    for s in range(2):
        np.testing.assert_array_equal(x[s, ..., 3:6], np.transpose(offs, (0, 2, 3, 1)).astype(np.float64))
    one = G.preprocess(bgr, None, offs, mean, std, xc=8, dtype=np.float32)
    assert one.shape == (1, B, H, W, 8) and one.dtype == np.float32
    np.testing.assert_array_equal(one[0, ..., 1], (bgr[..., 1].astype(np.float32) - np.float32(mean[1])) / np.float32(std[1]))
    a, b = rng.standard_normal((2, 3, 4, 8)).astype(np.float16), rng.standard_normal((2, 3, 4, 8)).astype(np.float16)
    np.testing.assert_array_equal(G.add(a, b), (torch.from_numpy(a).double() + torch.from_numpy(b).double()).numpy())
    c = G.copy(a)
    assert c is not a and c.dtype == a.dtype and np.array_equal(c, a)
