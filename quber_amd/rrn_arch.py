"""Parameter inventory + seeded initialiser of the Region Refinement Network of UOIS-Net-3D (reference uois/src/segmentation.py:248-292
``RegionRefinementNetwork(UNet_Encoder(4, fd), UNet_Decoder(1, fd), fg_module)``, uois/src/networks.py:12-56, 156-278; ``feature_dim`` 64
in ext_modules/uois/uoisnet3d.yaml).  Keys = that module's ``state_dict()`` keys; the reference's checkpoint holds them under 'model' with
the ``module.`` prefix of ``nn.DataParallel``, which ``load_checkpoint`` strips (dsn_arch.load_checkpoint with this file's inventory)."""
from collections import OrderedDict

import numpy as np

from . import dsn_arch

N_PARAMS_FD64 = 23070720           # RegionRefinementNetwork at feature_dim 64, counted from the reference module
FIRST = "encoder.layer1.layer1.conv1.weight"


def param_specs(feature_dim=64):
    fd = feature_dim
    s = OrderedDict()

    def cgr(n, ci, co, k=3):             # Conv2d_GN_ReLU
        s[n + ".conv1.weight"] = ((co, ci, k, k), "conv")
        s[n + ".gn1.weight"] = ((co,), "gn_w")
        s[n + ".gn1.bias"] = ((co,), "gn_b")

    def cgr2(n, ci, co):                 # Conv2d_GN_ReLUx2
        cgr(n + ".layer1", ci, co)
        cgr(n + ".layer2", co, co)

    def up(n, c, co):                    # Upsample_Concat_Conv2d_GN_ReLU_Multi_Branch, one encoder
        cgr(n + ".channel_reduction_layer", c, c // 2)
        cgr(n + ".conv_gn_relu", c, co)

    cgr2("encoder.layer1", 4, fd)
    cgr2("encoder.layer2", fd, 2 * fd)
    cgr2("encoder.layer3", 2 * fd, 4 * fd)
    cgr2("encoder.layer4", 4 * fd, 8 * fd)
    cgr("encoder.last_layer", 8 * fd, 16 * fd)
    cgr("decoder.fuse_layer", 16 * fd, 16 * fd, 1)
    up("decoder.layer1", 16 * fd, 8 * fd)
    up("decoder.layer2", 8 * fd, 4 * fd)
    up("decoder.layer3", 4 * fd, 2 * fd)
    up("decoder.layer4", 2 * fd, fd)
    cgr("decoder.layer5", fd, fd)
    s["decoder.last_conv.weight"] = ((fd, fd, 3, 3), "conv")
    s["decoder.last_conv.bias"] = ((fd,), "bias")
    s["fg_module.weight"] = ((1, fd, 1, 1), "head")
    if fd == 64:
        assert sum(int(np.prod(sh)) for sh, _ in s.values()) == N_PARAMS_FD64
    return s


def init_state_dict(seed=0, gain=0.7, feature_dim=64):
    """Seeded weights with non-trivial GroupNorm scales and shifts.  `gain` scales the He deviation of the convolutions
    (tests/golden_gen_rrn.py picks it)."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, (shape, kind) in param_specs(feature_dim).items():
        if kind == "conv":
            fan_in = shape[1] * shape[2] * shape[3]
            v = rng.normal(0, np.sqrt(2.0 / fan_in) * gain, shape)
        elif kind == "head":
            v = rng.normal(0, np.sqrt(1.0 / shape[1]), shape)
        elif kind == "gn_w":
            v = rng.uniform(0.6, 1.4, shape)
        elif kind in ("gn_b", "bias"):
            v = rng.normal(0, 0.1, shape)
        else:
            raise AssertionError(kind)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def load_checkpoint(path_or_dict):
    """A path to the reference's checkpoint (a dict with the state dict under 'model'), such a dict, or a bare state dict ->
    {key: float32 numpy array}, keys checked against ``param_specs`` of the feature_dim the first convolution has."""
    return dsn_arch.load_checkpoint(path_or_dict, specs=param_specs, what="Region Refinement Network")


def collapsed_head(sd):
    """decoder.last_conv followed by fg_module as one 3x3 feature_dim -> 1 filter (option key 54 = 1): float64 (w' [fd,3,3], b')."""
    wfg = np.asarray(sd["fg_module.weight"], np.float64).reshape(-1)
    w = np.asarray(sd["decoder.last_conv.weight"], np.float64)
    return np.einsum("o,ocyx->cyx", wfg, w), float(wfg @ np.asarray(sd["decoder.last_conv.bias"], np.float64))


def logit_threshold(t):
    """The probability threshold t of RRNWrapper.run_on_batch as the logit bound the device compares with: float32(log(t / (1 - t))),
    exactly 0 for t = 0.5."""
    t = float(t)
    if not 0.0 < t < 1.0:
        raise ValueError(f"threshold {t} outside (0, 1)")
    return np.float32(0.0) if t == 0.5 else np.float32(np.log(t / (1.0 - t)))
