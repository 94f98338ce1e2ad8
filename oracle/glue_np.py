"""Plain numpy float64 restatements of the glue operations between the convolutions (quber_amd/csrc/elementwise.hip), on NHWC
arrays.  Each is the operation as the network defines it, not the kernel's algorithm: tests/test_glue_reference_cpu.py pins them
against torch.nn.functional in float64, tests/test_gpu_glue.py holds the kernels against them.

Inputs are taken as they are stored (float32 / float16 / uint8) and widened to float64 exactly; results are float64 unless said."""
import numpy as np

F64 = np.float64
F32 = np.float32


def group_norm(x, groups, gamma, beta, eps=1e-5, relu=False, torch_f32_form=False):
    """GroupNorm over (H, W, C / groups) of x [B][H][W][C], moments in float64 (biased variance).
    torch_f32_form: mean and rstd rounded to float32, then `scale = rstd * gamma, bias = beta - mean * scale, y = x * scale + bias`
    in float32 - the form of torch's CPU kernel and of gn_apply_kernel - returned as float32.  It exists to measure how far ANY
    float32 implementation of that form lies from the float64 result, never as the expected value of a test."""
    B, H, W, C = x.shape
    cpg = C // groups
    xg = x.astype(F64).reshape(B, H * W, groups, cpg)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = 1.0 / np.sqrt(var + F64(eps))
    if torch_f32_form:
        mean_c = np.repeat(mean.astype(F32), cpg, axis=1)
        rstd_c = np.repeat(rstd.astype(F32), cpg, axis=1)
        scale = rstd_c * gamma.astype(F32)[None]
        bias = beta.astype(F32)[None] - mean_c * scale
        y = x.astype(F32) * scale[:, None, None, :] + bias[:, None, None, :]
        return np.maximum(y, F32(0)) if relu else y
    mean_c = np.repeat(mean, cpg, axis=1)[:, None, None, :]
    rstd_c = np.repeat(rstd, cpg, axis=1)[:, None, None, :]
    y = (x.astype(F64) - mean_c) * rstd_c * gamma.astype(F64) + beta.astype(F64)
    return np.maximum(y, 0.0) if relu else y


def group_sums(x, groups):
    """[B][groups][2]: sum and sum of squares per norm group, float64 (what gn_stats_kernel accumulates)."""
    B, H, W, C = x.shape
    xg = x.astype(F64).reshape(B, H * W, groups, C // groups)
    return np.stack([xg.sum(axis=(1, 3)), (xg * xg).sum(axis=(1, 3))], axis=-1)


def maxpool3x3s2(x):
    """3x3 / stride 2 / pad 1 max-pool of x [B][H][W][C]; the padding is -inf.  Exact: the result keeps x's dtype."""
    B, H, W, C = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    xp = np.full((B, 2 * OH + 1, 2 * OW + 1, C), -np.inf, dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.full((B, OH, OW, C), -np.inf, dtype=x.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + 2 * OH:2, dx:dx + 2 * OW:2])
    return out


def _source_f32(out_size, in_size, scale, fused=False):
    """torch's area_pixel_compute_source_index (align_corners=False) on its float path: index pair and weights in float32.
    `scale * (dst + 0.5) - 0.5` is rounded after the product and after the subtraction, as the source states it and as a build without
    contraction (the HIP library) evaluates it; fused = the same with one rounding (a host compiler that contracts it into an fma: some
    torch CPU builds) - an ulp of the coordinate apart wherever the product lies near a rounding boundary."""
    o = np.arange(out_size, dtype=F32)
    if fused:
        s = (F64(F32(scale)) * (o + F32(0.5)).astype(F64) - 0.5).astype(F32)     # (product of two float32: exact in float64)
    else:
        s = F32(scale) * (o + F32(0.5)) - F32(0.5)
    s = np.maximum(s, F32(0))
    i0 = np.minimum(s.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (s - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def _blend(x, OH, OW, sy, sx, ay, ax, fused=False):
    """bilinear blend in float64 of the rows `ay` / columns `ax` of x, weights from the float32 source coordinates"""
    y0, y1, hy, ly = _source_f32(OH, x.shape[ay], sy, fused)
    x0, x1, hx, lx = _source_f32(OW, x.shape[ax], sx, fused)
    xd = x.astype(F64)
    shape_y = [1] * x.ndim
    shape_y[ay] = OH
    shape_x = [1] * x.ndim
    shape_x[ax] = OW
    hy, ly = hy.astype(F64).reshape(shape_y), ly.astype(F64).reshape(shape_y)
    hx, lx = hx.astype(F64).reshape(shape_x), lx.astype(F64).reshape(shape_x)
    r0, r1 = np.take(xd, y0, axis=ay), np.take(xd, y1, axis=ay)
    top = hx * np.take(r0, x0, axis=ax) + lx * np.take(r0, x1, axis=ax)
    bot = hx * np.take(r1, x0, axis=ax) + lx * np.take(r1, x1, axis=ax)
    return hy * top + ly * bot


def bilinear(x, OH, OW, fused_coords=False):
    """F.interpolate(mode="bilinear", align_corners=False) of x [B][H][W][C] to OH x OW: source index and weight in float32 as
    torch's float path states them (scale = float(in) / float(out)), the blend in float64.  fused_coords: see _source_f32."""
    sy = F32(x.shape[1]) / F32(OH)
    sx = F32(x.shape[2]) / F32(OW)
    return _blend(x, OH, OW, sy, sx, 1, 2, fused_coords)


def upsample_logits(q, scale, OH, OW, mul_mask=0):
    """The planar x`scale` bilinear up-sampling of q [B][nch][h][w] (source coordinate from 1 / scale in float32), cropped to its
    top-left OH x OW; plane c of every frame is multiplied by `scale` when bit c of mul_mask is set."""
    B, nch, h, w = q.shape
    assert OH <= h * scale and OW <= w * scale
    inv = F32(1) / F32(scale)
    out = _blend(q, OH, OW, inv, inv, 2, 3)
    mul = np.array([float(scale) if (mul_mask >> c) & 1 else 1.0 for c in range(nch)], dtype=F64)
    return out * mul[None, :, None, None]


def avgpool(x):
    """mean over the pixels of x [B][H][W][C] -> [B][C]"""
    B, H, W, C = x.shape
    return x.astype(F64).reshape(B, H * W, C).mean(axis=1)


def predictor_logits(x, w, bias):
    """1x1 convolution: x [B][H][W][C], w [cout][C], bias [cout] -> [B][cout][H][W] (planar, as the logit buffer)"""
    return np.einsum("bhwc,kc->bkhw", x.astype(F64), w.astype(F64)) + bias.astype(F64)[None, :, None, None]


def softmax(z, axis):
    z = z.astype(F64)
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z.astype(F64)))


def preprocess(bgr, depth, offs, mean6, std6, xc=8, dtype=F64):
    """u8 bgr / depth [B][H][W][3] + offsets [B][3][H][W] (heat, off_y, off_x) -> the stream inputs [streams][B][H][W][xc]:
    [(img - mean) / std, heat, off_y, off_x, 0 ...]; depth None = one stream.  `dtype` float32 gives the kernel's own arithmetic."""
    imgs = [bgr] if depth is None else [bgr, depth]
    B, H, W, _ = bgr.shape
    out = np.zeros((len(imgs), B, H, W, xc), dtype=dtype)
    o = np.transpose(offs, (0, 2, 3, 1)).astype(dtype)
    for s, img in enumerate(imgs):
        m = np.asarray(mean6, dtype=dtype)[3 * s:3 * s + 3]
        d = np.asarray(std6, dtype=dtype)[3 * s:3 * s + 3]
        out[s, ..., 0:3] = (img.astype(dtype) - m) / d
        out[s, ..., 3:6] = o
    return out


def add(a, b):
    return a.astype(F64) + b.astype(F64)


def copy(a):
    return a.copy()
