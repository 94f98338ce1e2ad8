"""Parameter inventory + seeded initialiser of CGNet, the foreground net of the UOAIS base model (reference
foreground_segmentation/cgnet.py:275-368 ``Context_Guided_Network(classes=2, in_channel=4)`` with M = 3, N = 21; keys = that
module's ``state_dict()`` keys without ``num_batches_tracked``, which is what the reference's ``rgbd_fg.pth`` checkpoint holds
under 'model', foreground_segmentation/predictor.py:24-26)."""
from collections import OrderedDict

import numpy as np

M, N = 3, 21
STAGE2 = dict(channels=64, dilation=2, reduction=8)
STAGE3 = dict(channels=128, dilation=4, reduction=16)


def param_specs(classes=2, in_channel=4):
    s = OrderedDict()

    def conv(n, co, ci, k):
        s[n + ".conv.weight"] = ((co, ci, k, k), "conv")

    def bn(n, c):
        for t, kind in (("weight", "bn_w"), ("bias", "bn_b"), ("running_mean", "bn_m"), ("running_var", "bn_v")):
            s[f"{n}.{t}"] = ((c,), kind)

    def bnp(n, c):                       # BNPReLU / the tail of ConvBNPReLU: n.bn.*, n.act.weight
        bn(n + ".bn", c)
        s[n + ".act.weight"] = ((c,), "prelu")

    def cbp(n, co, ci, k):
        conv(n, co, ci, k)
        bnp(n, co)

    def fglo(n, c, r):
        s[n + ".fc.0.weight"] = ((c // r, c), "fc")
        s[n + ".fc.0.bias"] = ((c // r,), "fc_b")
        s[n + ".fc.2.weight"] = ((c, c // r), "fc")
        s[n + ".fc.2.bias"] = ((c,), "fc_b")

    def down(n, ci, co, r):              # ContextGuidedBlock_Down
        cbp(n + ".conv1x1", co, ci, 3)
        conv(n + ".F_loc", co, 1, 3)
        conv(n + ".F_sur", co, 1, 3)
        bn(n + ".bn", 2 * co)
        s[n + ".act.weight"] = ((2 * co,), "prelu")
        conv(n + ".reduce", co, 2 * co, 1)
        fglo(n + ".F_glo", co, r)

    def block(n, c, r):                  # ContextGuidedBlock
        cbp(n + ".conv1x1", c // 2, c, 1)
        conv(n + ".F_loc", c // 2, 1, 3)
        conv(n + ".F_sur", c // 2, 1, 3)
        bnp(n + ".bn_prelu", c)
        fglo(n + ".F_glo", c, r)

    for i, ci in enumerate((in_channel, 32, 32)):
        cbp(f"level1_{i}", 32, ci, 3)
    bnp("b1", 32 + in_channel)
    c2, c3 = STAGE2["channels"], STAGE3["channels"]
    down("level2_0", 32 + in_channel, c2, STAGE2["reduction"])
    for i in range(M - 1):
        block(f"level2.{i}", c2, STAGE2["reduction"])
    bnp("bn_prelu_2", 2 * c2 + in_channel)
    down("level3_0", 2 * c2 + in_channel, c3, STAGE3["reduction"])
    for i in range(N - 1):
        block(f"level3.{i}", c3, STAGE3["reduction"])
    bnp("bn_prelu_3", 2 * c3)
    conv("classifier.0", classes, 2 * c3, 1)
    return s


def init_state_dict(seed=0, gain=0.8, classes=2, in_channel=4):
    """Seeded weights with non-trivial BN statistics, PReLU slopes and FC biases.  `gain` scales the He deviation of the
    convolutions: 22 residual blocks deep, it is what keeps the activations - and with them the float32 error of any evaluation -
    bounded (tests/golden_gen_cgnet.py picks it)."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, (shape, kind) in param_specs(classes, in_channel).items():
        if kind == "conv":
            fan_in = shape[1] * shape[2] * shape[3]
            v = rng.normal(0, np.sqrt(2.0 / fan_in) * gain, shape)
        elif kind == "fc":
            v = rng.normal(0, np.sqrt(1.0 / shape[1]), shape)
        elif kind == "fc_b":
            v = rng.normal(0, 0.2, shape)
        elif kind == "bn_w":
            v = rng.uniform(0.6, 1.4, shape)
        elif kind in ("bn_b", "bn_m"):
            v = rng.normal(0, 0.1, shape)
        elif kind == "bn_v":
            v = rng.uniform(0.5, 1.5, shape)
        elif kind == "prelu":
            v = rng.uniform(0.1, 0.4, shape)
        else:
            raise AssertionError(kind)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out
