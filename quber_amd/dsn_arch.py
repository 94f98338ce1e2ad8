"""Parameter inventory + seeded initialiser of the Depth Seeding Network of UOIS-Net-3D (reference uois/src/segmentation.py:72-127
``DepthSeedingNetwork(UNetESP_Encoder(3, fd), UNetESP_Decoder(fd), fg_module, cd_module)``, uois/src/networks.py:12-154, 281-370;
``feature_dim`` 64 in ext_modules/uois/uoisnet3d.yaml).  Keys = that module's ``state_dict()`` keys; the reference's checkpoint holds
them under 'model' with the ``module.`` prefix of ``nn.DataParallel`` (segmentation.py:61, 126), which ``load_checkpoint`` strips."""
from collections import OrderedDict

import numpy as np

N_PARAMS_FD64 = 22336768           # DepthSeedingNetwork at feature_dim 64, counted from the reference module
DILATIONS = (1, 2, 4, 8, 16)


def esp_split(c):
    """ESPModule's channel split as the reference computes it: n = int(c / 5), n1 = c - 4 n -> (n, n1)"""
    n = int(c / 5)
    return n, c - 4 * n


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

    def esp(n, c, k):                    # ESPModule(c, c, fd, ksize=k)
        nn, n1 = esp_split(c)
        s[n + ".conv1.weight"] = ((nn, c, k, k), "conv")
        for d in DILATIONS:
            s[f"{n}.dilated{d}.weight"] = ((n1 if d == 1 else nn, nn, 3, 3), "esp")
        s[n + ".gn.weight"] = ((c,), "gn_w")
        s[n + ".gn.bias"] = ((c,), "gn_b")

    def up(n, c, co):                    # Upsample_Concat_Conv2d_GN_ReLU
        cgr(n + ".channel_reduction_layer", c, c // 2)
        cgr(n + ".conv_gn_relu", c, co)

    cgr2("encoder.layer1", 3, fd)
    cgr2("encoder.layer2", fd, 2 * fd)
    cgr("encoder.layer3a", 2 * fd, 4 * fd)
    esp("encoder.layer3b", 4 * fd, 3)
    cgr("encoder.layer4a", 4 * fd, 8 * fd)
    esp("encoder.layer4b", 8 * fd, 3)
    cgr("encoder.last_layer", 8 * fd, 16 * fd)
    esp("decoder.fuse_layer", 16 * fd, 1)
    up("decoder.layer1", 16 * fd, 8 * fd)
    up("decoder.layer2", 8 * fd, 4 * fd)
    up("decoder.layer3", 4 * fd, 2 * fd)
    up("decoder.layer4", 2 * fd, fd)
    cgr("decoder.layer5", fd, fd)
    s["decoder.last_conv.weight"] = ((fd, fd, 3, 3), "conv")
    s["decoder.last_conv.bias"] = ((fd,), "bias")
    s["fg_module.weight"] = ((3, fd, 1, 1), "head")
    s["cd_module.weight"] = ((3, fd, 1, 1), "head")
    if fd == 64:
        assert sum(int(np.prod(sh)) for sh, _ in s.values()) == N_PARAMS_FD64
    return s


def init_state_dict(seed=0, gain=0.7, feature_dim=64):
    """Seeded weights with non-trivial GroupNorm scales and shifts.  `gain` scales the He deviation of the convolutions
    (tests/golden_gen_dsn.py picks it)."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, (shape, kind) in param_specs(feature_dim).items():
        if kind in ("conv", "esp"):
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


def strip_module_prefix(sd):
    """A checkpoint's 'model' dict with or without DataParallel's ``module.`` prefix -> keys of ``param_specs``"""
    return OrderedDict((k[len("module."):] if k.startswith("module.") else k, v) for k, v in sd.items())


def load_checkpoint(path_or_dict, specs=None, what="Depth Seeding Network"):
    """A path to the reference's checkpoint (a dict with the state dict under 'model'), such a dict, or a bare state dict ->
    {key: float32 numpy array}, keys checked against ``param_specs`` of the feature_dim the first convolution has.  specs: another
    network's ``param_specs`` with the same first key (rrn_arch), `what` its name in the messages."""
    ck = path_or_dict
    if not isinstance(ck, dict):
        import torch
        ck = torch.load(ck, map_location="cpu", weights_only=False)
    if "model" in ck and isinstance(ck["model"], dict):
        ck = ck["model"]
    sd = OrderedDict()
    for k, v in strip_module_prefix(ck).items():
        sd[k] = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
    first = "encoder.layer1.layer1.conv1.weight"
    if first not in sd:
        raise KeyError(f"not a {what} state dict: '{first}' is missing")
    specs = (specs or param_specs)(int(sd[first].shape[0]))
    missing = [k for k in specs if k not in sd]
    if missing:
        raise KeyError(f"state dict lacks {len(missing)} keys, first '{missing[0]}'")
    for k, (shape, _) in specs.items():
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"'{k}' has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
    return OrderedDict((k, sd[k]) for k in specs)
