"""ORACLE (test infrastructure, never shipped): functional restatement of the LMFFNet foreground network used by the
reference's post-filter (eval/refiner_model.py:273-277 -> foreground_segmentation/predictor.py:57-99 ->
foreground_segmentation/lmffnet.py:283-341).  Weights are a dict keyed like the reference module's state_dict.

Staged: every launch of the HIP plan (csrc/plan_lmff.hip) has one function here, callable on its own on any tensor, in float32
or float64 (the dtype of the tensor and of the weight dict), and ``plan()`` lists the launches in the plan's order under the
plan's tap names.  ``forward`` is the composition of that list; tests/test_gpu_lmffnet.py evaluates the same list one entry at a
time on the device's own intermediates.

Pinned: the reference module imports here (torch only); tests/golden/lmffnet_*.npz hold its outputs for seeded
weights (oracle/gen_golden.py) and tests/test_oracle_golden.py checks this file against them (<= 1e-5)."""
import numpy as np
import torch
import torch.nn.functional as F

# dilation rates of the two SEM-B stacks (foreground_segmentation/lmffnet.py:299, 305); restated here, not imported
# from the product
SEM1_DIL = (2, 2, 2)
SEM2_DIL = (4, 4, 8, 8, 16, 16, 32, 32)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def preprocess(bgr_u8, depth_u8):
    """predictor.py:79-83 + eval/preprocess_utils.py:82-96: u8 HWC x2 -> f32 [1,6,H,W] (the BGR image is standardised
    with the RGB statistics, as the reference does)."""
    img = np.zeros(bgr_u8.shape, np.float32)
    for i in range(3):
        img[..., i] = (bgr_u8[..., i] / 255. - MEAN[i]) / STD[i]
    a = torch.from_numpy(img).permute(2, 0, 1).float()[None]
    d = torch.from_numpy(np.ascontiguousarray(depth_u8)).permute(2, 0, 1).float()[None] / 255
    return torch.cat([a, d], 1)


# ---- one function per launch of the plan: t = NCHW tensor, w = weight dict of t's dtype, n = key prefix ----
def bn_prelu(t, w, n):
    """BatchNorm2d(eps 1e-3, running statistics) + PReLU: keys n.bn.*, n.acti.weight"""
    t = F.batch_norm(t, w[n + ".bn.running_mean"], w[n + ".bn.running_var"], w[n + ".bn.weight"], w[n + ".bn.bias"],
                     False, 0.0, 1e-3)
    return F.prelu(t, w[n + ".acti.weight"])


def conv(t, w, n, stride=1, pad=0, dil=1, groups=1, bn=None):
    """n.conv.weight, then the BN + PReLU of key prefix `bn` when one is given"""
    o = F.conv2d(t, w[n + ".conv.weight"], None, stride, pad, dil, groups)
    return o if bn is None else bn_prelu(o, w, bn)


def dwconv(t, w, n, dil=1):
    """depthwise 3x3, dilation = padding, + BN + PReLU"""
    return conv(t, w, n, pad=dil, dil=dil, groups=t.shape[1], bn=n + ".bn_prelu")


def affine(a, w, n, add=None):
    """BN + PReLU of a tensor, or of the sum of two"""
    return bn_prelu(a if add is None else a + add, w, n)


def avg_pool(t):
    return F.avg_pool2d(t, 3, 2, 1)


def max_pool(t):
    return F.max_pool2d(t, 2, 2)


def pmca_weights(t, w, n):
    """lmffnet.py:172-191 up to the sigmoid: [B,C,H,W] -> channel weights [B,C]"""
    c = t.shape[1]
    o1 = F.conv2d(F.adaptive_avg_pool2d(t, (2, 2)), w[n + ".conv2x2.conv.weight"], None, 1, 0, 1, c)
    s = (o1 + F.adaptive_avg_pool2d(t, 1)).flatten(1)
    s = F.prelu(F.linear(s, w[n + ".SE_Block.fc.0.weight"]), w[n + ".SE_Block.fc.1.weight"])
    return torch.sigmoid(F.linear(s, w[n + ".SE_Block.fc.2.weight"]))


def channel_scale(t, s):
    return s[:, :, None, None] * t


def bilinear2(t):
    h, ww = t.shape[-2:]
    return F.interpolate(t, [h * 2, ww * 2], mode="bilinear", align_corners=False)


def mad_gate(o, att):
    """lmffnet.py:268-277: the class maps times the sigmoid of the attention logits"""
    return o * torch.sigmoid(att)


def final_upsample(q):
    """stride-4 maps -> frame size (the reference's x8 of the stride-8 size)"""
    h, ww = q.shape[-2:]
    return F.interpolate(q, [h * 4, ww * 4], mode="bilinear", align_corners=False)


class In:
    """An operand of a step: the channel concatenation of the named taps, or channels lo .. lo + n of it."""

    def __init__(self, *names, lo=0, n=None):
        self.names, self.lo, self.n = names, lo, n

    def take(self, get):
        ts = [get(k) for k in self.names]
        t = ts[0] if len(ts) == 1 else torch.cat(ts, 1)
        return t if self.n is None else t[:, self.lo:self.lo + self.n]


class Step:
    """One launch: out = fn(w, *operands).  kind names the kernel family; op = index of the plan op (quber_num_ops) it belongs to -
    the PMCA op and the last op are two launches each; key / bn / dil: what the launch's parameters are derived from."""

    def __init__(self, op, out, kind, ins, fn, key=None, bn=None, dil=1):
        self.op, self.out, self.kind, self.ins, self.fn, self.key, self.bn, self.dil = op, out, kind, ins, fn, key, bn, dil


# the concatenation buffers of the plan: tap name -> the taps written into it, in channel order (then zero pad channels)
CONCAT = {
    "A": ("Init_Block.init_conv.2", "inject_1"),
    "Bc": ("SEM_B_Block1.SEM_B_Block.SEM_Block_12.bn_relu_1", "FFM_B1.PMCA", "inject_2"),
    "Cc": ("SEM_B_Block2.SEM_B_Block.SEM_Block_27.bn_relu_1", "FFM_B2.PMCA", "inject_3"),
}
# the four short tap names the plan had before every op got one
ALIAS = {"ffm_a": "FFM_A.conv1x1", "d1": "downsample_1.bn_prelu", "ffm_b1": "FFM_B1.conv1x1", "ffm_b2": "FFM_B2.conv1x1"}


def plan():
    """The launches of csrc/plan_lmff.hip in its order, as Steps named by the plan's taps."""
    steps, nop = [], [0]

    def add(out, kind, ins, fn, same_op=False, **kw):
        if same_op:
            nop[0] -= 1
        steps.append(Step(nop[0], out, kind, ins, fn, **kw))
        nop[0] += 1
        return out

    def cv(n, src, bn=None, **kw):
        return add(n, "conv", [src], lambda w, t: conv(t, w, n, bn=bn, **kw), key=n, bn=bn)

    def dw(n, src, dil=1):
        return add(n, "dwconv", [src], lambda w, t: dwconv(t, w, n, dil), key=n, bn=n + ".bn_prelu", dil=dil)

    def af(n, src, addend=None):
        ins = [src] if addend is None else [src, addend]
        return add(n, "affine", ins, lambda w, a, b=None: affine(a, w, n, b), bn=n)

    def avg(n, src):
        return add(n, "avgpool", [src], lambda w, t: avg_pool(t))

    def pmca(n, src):
        add(n + ".weights", "pmca", [src], lambda w, t: pmca_weights(t, w, n), key=n)
        return add(n, "scale", [src, In(n + ".weights")], lambda w, t, s: channel_scale(t, s), same_op=True)

    def sem(n, src, d):
        c = 64 if "Block1" in n else 128
        t = cv(n + ".conv3x3", src, bn=n + ".conv3x3.bn_prelu", pad=1)
        left = dw(n + ".dconv_left", In(t, lo=0, n=c // 4), 1)
        right = dw(n + ".dconv_right", In(t, lo=c // 4, n=c // 4), d)
        v = cv(n + ".conv3x3_resume.conv3x3", In(left, right), bn=n + ".conv3x3_resume.conv3x3.bn_prelu", pad=1)
        r = cv(n + ".conv3x3_resume.conv1x1_resume", In(v))
        return af(n + ".bn_relu_1", In(r), src)

    x = In("X", lo=0, n=6)
    cur = x
    for i in range(3):
        n = f"Init_Block.init_conv.{i}"
        cur = In(cv(n, cur, bn=n + ".bn_prelu", stride=2 if i == 0 else 1, pad=1))
    avg("inject_1", x)
    af("FFM_A.bn_prelu", In(*CONCAT["A"]))
    cv("FFM_A.conv1x1", In("FFM_A.bn_prelu"))
    cv("downsample_1.conv3x3", In("FFM_A.conv1x1"), stride=2, pad=1)
    add("downsample_1.maxpool", "maxpool", [In("FFM_A.conv1x1")], lambda w, t: max_pool(t))
    d1 = In(af("downsample_1.bn_prelu", In("downsample_1.conv3x3", "downsample_1.maxpool")))
    cur = d1
    for i, d in enumerate(SEM1_DIL):
        cur = In(sem(f"SEM_B_Block1.SEM_B_Block.SEM_Block_1{i}", cur, d))
    pmca("FFM_B1.PMCA", d1)
    avg("inject_2.0", x)
    avg("inject_2", In("inject_2.0"))
    af("FFM_B1.bn_prelu", In(*CONCAT["Bc"]))
    cv("FFM_B1.conv1x1", In("FFM_B1.bn_prelu"))
    d2 = In(cv("downsample_2.conv3x3", In("FFM_B1.conv1x1"), bn="downsample_2.bn_prelu", stride=2, pad=1))
    cur = d2
    for i, d in enumerate(SEM2_DIL):
        cur = In(sem(f"SEM_B_Block2.SEM_B_Block.SEM_Block_2{i}", cur, d))
    pmca("FFM_B2.PMCA", d2)
    avg("inject_3.0", x)
    avg("inject_3.1", In("inject_3.0"))
    avg("inject_3", In("inject_3.1"))
    af("FFM_B2.bn_prelu", In(*CONCAT["Cc"]))
    cv("FFM_B2.conv1x1", In("FFM_B2.bn_prelu"))
    # MAD (lmffnet.py:232-280)
    cv("MAD.mid_layer_1x1", In("FFM_B1.conv1x1"))
    cv("MAD.deep_layer_1x1", In("FFM_B2.conv1x1"))
    add("MAD.up_deep", "bilinear", [In("MAD.deep_layer_1x1")], lambda w, t: bilinear2(t))
    dw("MAD.DwConv1", In("MAD.mid_layer_1x1", "MAD.up_deep"))
    cv("MAD.PwConv1", In("MAD.DwConv1"))
    dw("MAD.DwConv2", In("FFM_B2.conv1x1"))
    cv("MAD.PwConv2", In("MAD.DwConv2"))
    add("MAD.up_out", "bilinear", [In("MAD.PwConv2")], lambda w, t: bilinear2(t))
    add("MAD.gate", "gate", [In("MAD.up_out"), In("MAD.PwConv1")], lambda w, o, a: mad_gate(o, a))
    add("logits", "upsample", [In("MAD.gate")], lambda w, q: final_upsample(q), same_op=True)
    return steps


def forward(x, w, taps=None):
    """[B,6,H,W] -> logits [B,3,H,W]; `taps`, when given, receives every intermediate under the plan's tap names (NCHW; the PMCA
    weights as [B,C]), the three concatenation buffers without their pad channels and the four short names."""
    env = {"X": x}
    for st in plan():
        env[st.out] = st.fn(w, *[i.take(env.__getitem__) for i in st.ins])
    if taps is not None:
        taps.update(env)
        taps.update({k: torch.cat([env[n] for n in v], 1) for k, v in CONCAT.items()})
        taps.update({k: env[v] for k, v in ALIAS.items()})
    return env["logits"]


def foreground_mask(logits):
    """predictor.py:85,98: argmax over the 3 classes, foreground = class 2."""
    return (np.argmax(logits, axis=0) == 2)


def overlap_filter(masks, fg, ratio=0.3):
    """eval/refiner_model.py:274-277: keep masks whose foreground overlap exceeds 30 %."""
    return [m for m in masks if np.sum(np.bitwise_and(m, fg)) / np.sum(m) > ratio]
