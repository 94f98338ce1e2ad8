"""Test infrastructure: a functional restatement of the Depth Seeding Network of UOIS-Net-3D (reference uois/src/segmentation.py:72-127
DepthSeedingNetwork over uois/src/networks.py UNetESP_Encoder / UNetESP_Decoder; input cleaning of eval/base_model.py:496-498; the
foreground rule of segmentation.py:232-233).  Weights are a dict keyed like that module's state_dict; feature_dim is the first
convolution's output channel count and the GroupNorm group count.

Staged: every launch of the HIP plan (csrc/plan_dsn.hip) has one Step per tensor it writes, a function of named taps that runs in
float32 or float64 (the dtype of the tensors and of the weight dict); ``plan(fused)`` lists them in the plan's order under the plan's
tap names, ``ops(fused)`` the plan's op names.  ``forward`` composes the list.  tests/golden/dsn_scene_*.npz hold the outputs of the
imported reference module for seeded weights (tests/golden_gen_dsn.py); tests/test_dsn_cpu.py holds this file to them."""
import numpy as np
import torch
import torch.nn.functional as F

from quber_amd.dsn_arch import DILATIONS, esp_split


def synth_xyz(h, w, seed):
    """A synthetic tilted depth surface with a few boxes on it and a few NaN pixels -> f32 [3,h,w] (x, y, z in metres)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 0.6 + 0.5 * ys / h + 0.15 * xs / w
    for _ in range(4):
        cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
        ry, rx = rng.uniform(0.08, 0.2) * h, rng.uniform(0.08, 0.2) * w
        z = np.where((np.abs(ys - cy) < ry) & (np.abs(xs - cx) < rx), z - rng.uniform(0.05, 0.15), z)
    z = z + rng.normal(0, 0.002, z.shape)
    fx = fy = 1.1 * w
    xyz = np.stack([(xs - w / 2) / fx * z, (ys - h / 2) / fy * z, z]).astype(np.float32)
    for _ in range(6):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        xyz[:, y:y + 2, x:x + 3] = np.nan
    return xyz


# ---- the pieces: t = NCHW tensor, w = weight dict of t's dtype ----
def clean(xyz, negate_y=True):
    """eval/base_model.py:496-498: NaN -> 0, then y times -1"""
    o = torch.where(torch.isnan(xyz), torch.zeros_like(xyz), xyz)
    if negate_y:
        o = torch.cat([o[:, 0:1], o[:, 1:2] * -1, o[:, 2:3]], 1)
    return o


def conv(t, w, n, dil=1):
    """n.weight [+ n.bias]; padding = dilation for a 3x3, none for a 1x1"""
    k = w[n + ".weight"].shape[-1]
    return F.conv2d(t, w[n + ".weight"], w.get(n + ".bias"), 1, dil if k == 3 else 0, dil)


def gn_relu(t, w, n):
    """GroupNorm(feature_dim groups, eps 1e-5) + ReLU under n.{weight, bias}"""
    return F.relu(F.group_norm(t, feature_dim(w), w[n + ".weight"], w[n + ".bias"], 1e-5))


def esp_combine(d, x=None):
    """networks.py:115-125: [d1 | d2 | d2 + d4 | (d2 + d4) + d8 | ((d2 + d4) + d8) + d16] [+ x]"""
    parts, run = [d[0]], None
    for t in d[1:]:
        run = t if run is None else run + t
        parts.append(run)
    o = torch.cat(parts, 1)
    return o if x is None else x + o


def esp_branches(t, x, w, n):
    return esp_combine([conv(t, w, f"{n}.dilated{d}", d) for d in DILATIONS], x)


def max_pool(t):
    return F.max_pool2d(t, 2, 2)


def upsample2(t):
    return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)


def head(t, w, n):
    return F.conv2d(t, w[n + ".weight"])


def classes(logits):
    """the first maximal logit -> u8 [B,h,w]"""
    return torch.argmax(logits, 1).to(torch.uint8)


def feature_dim(w):
    return int(w["encoder.layer1.layer1.conv1.weight"].shape[0])


class In:
    """An operand of a step: the channel concatenation of the named taps."""

    def __init__(self, *names):
        self.names = names

    def take(self, get):
        ts = [get(k) for k in self.names]
        return ts[0] if len(ts) == 1 else torch.cat(ts, 1)


class Step:
    """One checkable result of a launch: out = fn(w, *operands).  kind names the kernel family, op the plan op that writes it; key: the
    weight key prefix of the launch, dil its dilation."""

    def __init__(self, op, out, kind, ins, fn, key=None, dil=1):
        self.op, self.out, self.kind, self.ins, self.fn, self.key, self.dil = op, out, kind, ins, fn, key, dil


# the concatenation buffers of the plan: tap name -> the taps written into it, in channel order
CONCAT = {
    "cat1": ("decoder.layer1.upsample", "encoder.layer4b.gn"),
    "cat2": ("decoder.layer2.upsample", "encoder.layer3b.gn"),
    "cat3": ("decoder.layer3.upsample", "encoder.layer2.layer2.gn1"),
    "cat4": ("decoder.layer4.upsample", "encoder.layer1.layer2.gn1"),
}
ESP = ("encoder.layer3b", "encoder.layer4b", "decoder.fuse_layer")
OUTPUTS = ("fg_logits", "center_offsets", "votes", "fg_classes", "fg")


def _build(fused, negate_y=True):
    steps, names = [], []

    def add(op, out, kind, ins, fn, **kw):
        if not names or names[-1] != op:
            names.append(op)
        steps.append(Step(op, out, kind, [i if isinstance(i, In) else In(i) for i in ins], fn, **kw))
        return out

    def cv(n, src, dil=1):
        return add(n, n, "conv", [src], lambda w, t: conv(t, w, n, dil), key=n, dil=dil)

    def gn(n, src):
        return add(n, n, "gn", [src], lambda w, t: gn_relu(t, w, n), key=n)

    def cgr(n, src):
        return gn(n + ".gn1", cv(n + ".conv1", src))

    def pool(n, src):
        return add(n, n, "pool", [src], lambda w, t: max_pool(t))

    def esp(n, x):
        t = cv(n + ".conv1", x)
        if fused:
            add(n + ".branches", n + ".sum", "esp", [t, x], lambda w, tt, xx: esp_branches(tt, xx, w, n), key=n)
        else:
            ds = [cv(f"{n}.dilated{d}", t, d) for d in DILATIONS]
            add(n + ".merge", n + ".sum", "merge", ds + [x], lambda w, *a: esp_combine(list(a[:5]), a[5]), key=n)
        return gn(n + ".gn", n + ".sum")

    def up(n, x1, skip):
        r = cgr(n + ".channel_reduction_layer", x1)
        u = add(n + ".upsample", n + ".upsample", "bilinear", [r], lambda w, t: upsample2(t))
        return cgr(n + ".conv_gn_relu", In(u, skip))

    add("pack", "xyz", "pack", ["input"], lambda w, t: clean(t, negate_y))
    add("pack", "X", "pack8", ["xyz"], lambda w, t: torch.cat([t, torch.zeros_like(t[:, :1]).expand(-1, 5, -1, -1)], 1))
    add("encoder.layer1.layer1.conv1", "encoder.layer1.layer1.conv1", "conv", ["xyz"], lambda w, t: conv(t, w, "encoder.layer1.layer1.conv1"),
        key="encoder.layer1.layer1.conv1")
    a1 = gn("encoder.layer1.layer1.gn1", "encoder.layer1.layer1.conv1")
    x1 = cgr("encoder.layer1.layer2", a1)
    x2 = cgr("encoder.layer2.layer2", cgr("encoder.layer2.layer1", pool("pool1", x1)))
    x3 = esp("encoder.layer3b", cgr("encoder.layer3a", pool("pool2", x2)))
    x4 = esp("encoder.layer4b", cgr("encoder.layer4a", pool("pool3", x3)))
    x5 = cgr("encoder.last_layer", pool("pool4", x4))
    o = esp("decoder.fuse_layer", x5)
    for i, skip in ((1, x4), (2, x3), (3, x2), (4, x1)):
        o = up("decoder.layer%d" % i, o, skip)
    o = cgr("decoder.layer5", o)
    f = cv("decoder.last_conv", o)
    add("head", "fg_logits", "head", [f], lambda w, t: head(t, w, "fg_module"), key="fg_module")
    add("head", "center_offsets", "head", [f], lambda w, t: head(t, w, "cd_module"), key="cd_module")
    add("head", "votes", "votes", ["xyz", "center_offsets"], lambda w, a, b: a + b)
    add("head", "fg_classes", "classes", ["fg_logits"], lambda w, t: classes(t))
    add("head", "fg", "fg", ["fg_classes"], lambda w, t: (t == 2).to(torch.uint8))
    return steps, names


def plan(fused=True, negate_y=True):
    """The checkable results of csrc/plan_dsn.hip's launches in its order, named by the plan's taps.  fused: option dsn_fused."""
    return _build(fused, negate_y)[0]


def ops(fused=True):
    """The op names of the plan (quber_op_info), in order."""
    return _build(fused)[1]


def forward(xyz, w, taps=None, fused=True, negate_y=True):
    """raw xyz [B,3,h,w] -> (fg_logits, center_offsets) [B,3,h,w] each; `taps`, when given, receives every intermediate under the plan's
    tap names (NCHW) and the four concatenation buffers."""
    env = {"input": xyz}
    for st in plan(fused, negate_y):
        env[st.out] = st.fn(w, *[i.take(env.__getitem__) for i in st.ins])
    if taps is not None:
        taps.update(env)
        taps.update({k: torch.cat([env[n] for n in v], 1) for k, v in CONCAT.items()})
    return env["fg_logits"], env["center_offsets"]
