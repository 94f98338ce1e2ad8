"""Test infrastructure: a functional restatement of the Region Refinement Network of UOIS-Net-3D (reference uois/src/segmentation.py:248-266
RegionRefinementNetwork over uois/src/networks.py UNet_Encoder(4, fd) / UNet_Decoder(1, fd)).  Weights are a dict keyed like that
module's state_dict; feature_dim is the first convolution's output channel count and the GroupNorm group count.

Staged like tests/dsn_torch.py, whose pieces it uses: every launch of the HIP plan (csrc/plan_rrn.hip) has one Step per tensor it
writes, a function of named taps that runs in float32 or float64; ``plan(head)`` lists them in the plan's order under the plan's tap
names, ``ops(head)`` the plan's op names (head: option key 54).  tests/golden/rrn_net_*.npz hold the outputs of the imported reference
module for seeded weights (tests/golden_gen_rrn.py); tests/test_rrn_cpu.py holds this file to them."""
import numpy as np
import torch
import torch.nn.functional as F

from dsn_torch import In, Step, conv, gn_relu, max_pool, upsample2

CONCAT = {
    "cat1": ("decoder.layer1.upsample", "encoder.layer4.layer2.gn1"),
    "cat2": ("decoder.layer2.upsample", "encoder.layer3.layer2.gn1"),
    "cat3": ("decoder.layer3.upsample", "encoder.layer2.layer2.gn1"),
    "cat4": ("decoder.layer4.upsample", "encoder.layer1.layer2.gn1"),
}
OUTPUTS = ("logits",)


def synth_crops(n, S, seed):
    """n crops: smooth standardised-range colour fields f32 [n,3,S,S] and a blob mask u8 [n,S,S] each"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:S, 0:S].astype(np.float64) / S
    rgb = np.zeros((n, 3, S, S), np.float32)
    mask = np.zeros((n, S, S), np.uint8)
    for i in range(n):
        for c in range(3):
            a, b, p, q = rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(1, 4), rng.uniform(1, 4)
            rgb[i, c] = a * np.sin(p * np.pi * xs + c) * np.cos(q * np.pi * ys) + b + rng.normal(0, 0.05, (S, S))
        cy, cx, ry, rx = rng.uniform(0.35, 0.65), rng.uniform(0.35, 0.65), rng.uniform(0.15, 0.35), rng.uniform(0.15, 0.35)
        mask[i] = (((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 < 1).astype(np.uint8)
    return rgb, mask


def pack(rgb, mask):
    """segmentation.py:262-264: [rgb | mask as 0 / 1] -> [n,4,S,S]"""
    return torch.cat([rgb, (mask != 0).to(rgb.dtype)[:, None]], 1)


def collapsed(w):
    """decoder.last_conv then fg_module as one 3x3 filter, in w's dtype from float64: (w' [1,fd,3,3], b' [1])"""
    wfg = w["fg_module.weight"].double().reshape(-1)
    w9 = torch.einsum("o,ocyx->cyx", wfg, w["decoder.last_conv.weight"].double())[None]
    b = (wfg @ w["decoder.last_conv.bias"].double()).reshape(1)
    dt = w["fg_module.weight"].dtype
    return w9.to(dt), b.to(dt)


def head3(t, w):
    w9, b = collapsed(w)
    return F.conv2d(t, w9, b, 1, 1)[:, 0]


def _build(head):
    steps, names = [], []

    def add(op, out, kind, ins, fn, **kw):
        if not names or names[-1] != op:
            names.append(op)
        steps.append(Step(op, out, kind, [i if isinstance(i, In) else In(i) for i in ins], fn, **kw))
        return out

    def cv(n, src):
        return add(n, n, "conv", [src], lambda w, t: conv(t, w, n), key=n)

    def gn(n, src):
        return add(n, n, "gn", [src], lambda w, t: gn_relu(t, w, n), key=n)

    def cgr(n, src):
        return gn(n + ".gn1", cv(n + ".conv1", src))

    def cgr2(n, src):
        return cgr(n + ".layer2", cgr(n + ".layer1", src))

    def pool(n, src):
        return add(n, n, "pool", [src], lambda w, t: max_pool(t))

    def up(n, x1, skip):
        r = cgr(n + ".channel_reduction_layer", x1)
        u = add(n + ".upsample", n + ".upsample", "bilinear", [r], lambda w, t: upsample2(t))
        return cgr(n + ".conv_gn_relu", In(u, skip))

    add("pack", "X", "pack8", ["rgb", "mask"], lambda w, a, m: torch.cat([pack(a, m), torch.zeros_like(a[:, :1]).expand(-1, 4, -1, -1)], 1))
    add("encoder.layer1.layer1.conv1", "encoder.layer1.layer1.conv1", "conv", ["X"], lambda w, t: conv(t[:, :4], w, "encoder.layer1.layer1.conv1"),
        key="encoder.layer1.layer1.conv1")
    a1 = gn("encoder.layer1.layer1.gn1", "encoder.layer1.layer1.conv1")
    x1 = cgr("encoder.layer1.layer2", a1)
    x2 = cgr2("encoder.layer2", pool("pool1", x1))
    x3 = cgr2("encoder.layer3", pool("pool2", x2))
    x4 = cgr2("encoder.layer4", pool("pool3", x3))
    x5 = cgr("encoder.last_layer", pool("pool4", x4))
    o = cgr("decoder.fuse_layer", x5)
    for i, skip in ((1, x4), (2, x3), (3, x2), (4, x1)):
        o = up("decoder.layer%d" % i, o, skip)
    o = cgr("decoder.layer5", o)
    if head:
        add("head3", "logits", "head3", [o], lambda w, t: head3(t, w), key="fg_module")
    else:
        f = cv("decoder.last_conv", o)
        add("head", "logits", "head", [f], lambda w, t: F.conv2d(t, w["fg_module.weight"])[:, 0], key="fg_module")
    return steps, names


def plan(head=0):
    """The checkable results of csrc/plan_rrn.hip's launches in its order, named by the plan's taps.  head: option rrn_head."""
    return _build(head)[0]


def ops(head=0):
    """The op names of the plan (quber_op_info), in order."""
    return _build(head)[1]


def forward(rgb, mask, w, taps=None, head=0):
    """standardised crops [n,3,S,S] + mask [n,S,S] -> logits [n,S,S]; `taps`, when given, receives every intermediate under the plan's tap
    names (NCHW) and the four concatenation buffers.  head = 0 is the reference's own order of operations."""
    env = {"rgb": rgb, "mask": mask}
    for st in plan(head):
        env[st.out] = st.fn(w, *[i.take(env.__getitem__) for i in st.ins])
    if taps is not None:
        taps.update(env)
        taps.update({k: torch.cat([env[n] for n in v], 1) for k, v in CONCAT.items()})
    return env["logits"]
