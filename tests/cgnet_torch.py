"""Test infrastructure: a functional restatement of CGNet, the foreground network of the UOAIS base model, and of the filter
built on it (reference eval/base_model.py:191-219 -> foreground_segmentation/predictor.py:21-52 ->
foreground_segmentation/cgnet.py:275-368, classes = 2, in_channel = 4, M = 3, N = 21).  Weights are a dict keyed like that
module's state_dict.

Staged: every launch of the HIP plan (csrc/plan_cgnet.hip) has one Step here, a function of named taps that runs in float32 or
float64 (the dtype of the tensors and of the weight dict); ``plan(fused)`` lists them in the plan's order under the plan's tap
names, ``ops(fused)`` the plan's op names.  ``forward`` composes the list.  tests/golden/cgnet_scene_*.npz hold the outputs of the
imported reference module for seeded weights (tests/golden_gen_cgnet.py); tests/test_cgnet_cpu.py holds this file to them."""
import numpy as np
import torch
import torch.nn.functional as F

from quber_amd.cgnet_arch import M, N, STAGE2, STAGE3

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def preprocess(bgr, depth):
    """predictor.py:43-46: u8 [h,w,3] x2 -> f32 [1,4,h,w].  Channel i of the BGR image is standardised with entry i of the RGB
    statistics in float64 and stored as float32 (standardize_image on a cv2.imread image); depth channel 0 is divided by 255."""
    img = np.zeros(bgr.shape, np.float32)
    for i in range(3):
        img[..., i] = (bgr[..., i] / 255. - MEAN[i]) / STD[i]
    a = torch.from_numpy(img).permute(2, 0, 1).float()[None]
    d = torch.from_numpy(np.ascontiguousarray(depth[:, :, 0:1])).permute(2, 0, 1).float()[None] / 255
    return torch.cat([a, d], 1)


# ---- the pieces: t = NCHW tensor, w = weight dict of t's dtype ----
def bn(t, w, n, lo=0, c=None):
    """BatchNorm2d(eps 1e-3) with running statistics, keys n.*; channels lo .. lo + c of it"""
    sl = slice(lo, None if c is None else lo + c)
    return F.batch_norm(t, w[n + ".running_mean"][sl], w[n + ".running_var"][sl], w[n + ".weight"][sl], w[n + ".bias"][sl], False, 0.0, 1e-3)


def bn_prelu(t, w, n, lo=0, c=None):
    """keys n.bn.*, n.act.weight"""
    sl = slice(lo, None if c is None else lo + c)
    return F.prelu(bn(t, w, n + ".bn", lo, c), w[n + ".act.weight"][sl])


def conv(t, w, n, stride=1, pad=0, act=None):
    """n.conv.weight, then the BN + PReLU under key prefix `act` when one is given"""
    o = F.conv2d(t, w[n + ".conv.weight"], None, stride, pad)
    return o if act is None else bn_prelu(o, w, act)


def dwconv(t, w, n, dil, act, lo):
    """depthwise 3x3, dilation = padding, then channels lo.. of the BN + PReLU `act` of the concatenation it is written into"""
    c = t.shape[1]
    return bn_prelu(F.conv2d(t, w[n + ".conv.weight"], None, 1, dil, dil, c), w, act, lo, c)


def joint(x, w, n, dil):
    """the first half of a CG block: 1x1 + BN + PReLU to half the channels, both depthwise 3x3, concatenate, BN + PReLU"""
    t = conv(x, w, n + ".conv1x1", act=n + ".conv1x1")
    h = t.shape[1]
    return torch.cat([dwconv(t, w, n + ".F_loc", 1, n + ".bn_prelu", 0), dwconv(t, w, n + ".F_sur", dil, n + ".bn_prelu", h)], 1)


def mean(t):
    return t.mean((2, 3))


def gate(m, w, n):
    """FGlo's two fully connected layers: [B,C] -> [B,C]"""
    hid = F.relu(F.linear(m, w[n + ".fc.0.weight"], w[n + ".fc.0.bias"]))
    return torch.sigmoid(F.linear(hid, w[n + ".fc.2.weight"], w[n + ".fc.2.bias"]))


def apply(joi, y, x=None):
    o = joi * y[:, :, None, None]
    return o if x is None else x + o


def avg_pool(t):
    return F.avg_pool2d(t, 3, 2, 1)


def upsample8(t):
    h, ww = t.shape[-2:]
    return F.interpolate(t, [h * 8, ww * 8], mode="bilinear", align_corners=False)


class In:
    """An operand of a step: the channel concatenation of the named taps, or channels lo .. lo + n of it."""

    def __init__(self, *names, lo=0, n=None):
        self.names, self.lo, self.n = names, lo, n

    def take(self, get):
        ts = [get(k) for k in self.names]
        t = ts[0] if len(ts) == 1 else torch.cat(ts, 1)
        return t if self.n is None else t[:, self.lo:self.lo + self.n]


class Step:
    """One checkable result of a launch: out = fn(w, *operands).  kind names the kernel family, op the plan op that writes it;
    key / act / lo / dil: what the launch's parameters derive from (act = BN + PReLU key prefix, lo = first channel of it)."""

    def __init__(self, op, out, kind, ins, fn, key=None, act=None, lo=0, dil=1):
        self.op, self.out, self.kind, self.ins, self.fn, self.key, self.act, self.lo, self.dil = op, out, kind, ins, fn, key, act, lo, dil


# the concatenation buffers of the plan: tap name -> the taps written into it, in channel order (then zero pad channels)
CONCAT = {
    "A": ("level1_2", "inject_1"),
    "Bc": ("level2.%d" % (M - 2), "level2_0", "inject_2"),
    "Cc": ("level3_0", "level3.%d" % (N - 2)),
}


def _build(fused):
    steps, names = [], []

    def add(op, out, kind, ins, fn, **kw):
        if not names or names[-1] != op:
            names.append(op)
        steps.append(Step(op, out, kind, ins, fn, **kw))
        return out

    def cv(n, src, act=None, **kw):
        return add(n, n, "conv", [src], lambda w, t: conv(t, w, n, act=act, **kw), key=n, act=act)

    def dw(n, src, dil, act, lo):
        return add(n, n, "dwconv", [src], lambda w, t: dwconv(t, w, n, dil, act, lo), key=n, act=act, lo=lo, dil=dil)

    def af(n, src):
        return add(n, n, "affine", [src], lambda w, t: bn_prelu(t, w, n), act=n)

    def avg(n, src):
        return add(n, n, "avgpool", [src], lambda w, t: avg_pool(t))

    def glo(n, feat, x):
        """global pool, FC gate, channel scale [+ residual]: the apply launch, which reduces the tile sums its producer left"""
        g = n + ".F_glo"
        add(n, g + ".mean", "mean", [feat], lambda w, t: mean(t))
        add(n, g + ".y", "gate", [In(g + ".mean")], lambda w, m: gate(m, w, g), key=g)
        ins = [feat, In(g + ".y")] + ([] if x is None else [x])
        return add(n, n, "apply", ins, lambda w, j, y, r=None: apply(j, y, r))

    def down(n, src, dil):
        co = STAGE2["channels"] if n == "level2_0" else STAGE3["channels"]
        t = In(cv(n + ".conv1x1", src, act=n + ".conv1x1", stride=2, pad=1))
        dw(n + ".F_loc", t, 1, n, 0)
        dw(n + ".F_sur", t, dil, n, co)
        r = In(cv(n + ".reduce", In(n + ".F_loc", n + ".F_sur")))
        names.append(n + ".F_glo.sums")
        return In(glo(n, r, None))

    def block(n, src, dil):
        c = STAGE2["channels"] if n.startswith("level2") else STAGE3["channels"]
        if fused:
            add(n + ".joi", n + ".joi", "joint", [src], lambda w, t: joint(t, w, n, dil), key=n, dil=dil)
        else:
            t = In(cv(n + ".conv1x1", src, act=n + ".conv1x1"))
            dw(n + ".F_loc", t, 1, n + ".bn_prelu", 0)
            dw(n + ".F_sur", t, dil, n + ".bn_prelu", c // 2)
            add(n + ".F_sur", n + ".joi", "concat", [In(n + ".F_loc", n + ".F_sur")], lambda w, t: t)
            names.append(n + ".F_glo.sums")
        return In(glo(n, In(n + ".joi"), src))

    x = In("X", lo=0, n=4)
    cur = x
    for i in range(3):
        n = "level1_%d" % i
        cur = In(cv(n, cur, act=n, stride=2 if i == 0 else 1, pad=1))
    avg("inject_1", x)
    af("b1", In(*CONCAT["A"]))
    cur = down("level2_0", In("b1"), STAGE2["dilation"])
    for i in range(M - 1):
        cur = block("level2.%d" % i, cur, STAGE2["dilation"])
    avg("inject_2.0", x)
    avg("inject_2", In("inject_2.0"))
    af("bn_prelu_2", In(*CONCAT["Bc"]))
    cur = down("level3_0", In("bn_prelu_2"), STAGE3["dilation"])
    for i in range(N - 1):
        cur = block("level3.%d" % i, cur, STAGE3["dilation"])
    af("bn_prelu_3", In(*CONCAT["Cc"]))
    cv("classifier.0", In("bn_prelu_3"))
    add("logits", "logits", "upsample", [In("classifier.0")], lambda w, t: upsample8(t))
    return steps, names


def plan(fused=True):
    """The checkable results of csrc/plan_cgnet.hip's launches in its order, named by the plan's taps.  fused: option cgnet_fused."""
    return _build(fused)[0]


def ops(fused=True):
    """The op names of the plan (quber_op_info), in order.  A ``*.F_glo.sums`` op writes only the tile sums that the op after it
    reduces: it is checked through that op's ``.F_glo.mean``."""
    return _build(fused)[1]


def forward(x, w, taps=None, fused=True):
    """[B,4,h,w] -> logits [B,2,h,w]; `taps`, when given, receives every intermediate under the plan's tap names (NCHW; means and
    gates as [B,C]) and the three concatenation buffers without their pad channels."""
    env = {"X": x}
    for st in plan(fused):
        env[st.out] = st.fn(w, *[i.take(env.__getitem__) for i in st.ins])
    if taps is not None:
        taps.update(env)
        taps.update({k: torch.cat([env[n] for n in v], 1) for k, v in CONCAT.items()})
    return env["logits"]


def foreground_mask(logits):
    """predictor.py:49: argmax over the two class planes [2,h,w] (the first maximum wins), foreground = class 1 -> u8 [h,w]"""
    return np.asarray(np.argmax(logits, axis=0), dtype=np.uint8)


def upsample_nearest(img, oh, ow):
    """cv2.resize(img, (ow, oh), interpolation=cv2.INTER_NEAREST): src = floor(dst * scale), clipped, with OpenCV's float64
    scale = 1 / (dst size / src size)"""
    h, w = img.shape[:2]
    ys = np.minimum(np.floor(np.arange(oh) * (1.0 / (oh / h))).astype(np.int64), h - 1)
    xs = np.minimum(np.floor(np.arange(ow) * (1.0 / (ow / w))).astype(np.int64), w - 1)
    return img[ys][:, xs]


def uoais_filter(masks, fg, ratio=0.5):
    """eval/base_model.py:210-216: empty masks are skipped, a mask is kept where |mask & fg| / |mask| > 0.5 (float64).
    -> (kept masks, their indices)"""
    kept, index = [], []
    fgb = fg.astype(bool)
    for i, m in enumerate(masks):
        mb = m.astype(bool)
        if np.sum(mb) == 0:
            continue
        if np.sum(np.bitwise_and(mb, fgb)) / np.sum(mb) > ratio:
            kept.append(m)
            index.append(i)
    return kept, index
