"""Generator of tests/golden/dsn_scene_*.npz.  Not collected by pytest; run by hand on a CPU machine that has the reference:

    python tests/golden_gen_dsn.py --reference /path/to/reference/ext_modules

It imports the reference's uois/src/networks.py by path (torch only; an empty stand-in is registered for its ``.util`` import, which
the network classes never use), composes UNetESP_Encoder(3, 64), UNetESP_Decoder(64) and the two bias-free 1x1 heads under the
attribute names of uois/src/segmentation.py's DepthSeedingNetwork, loads dsn_arch.init_state_dict(seed, gain) with strict=True and
runs it in float32 and float64 on dsn_torch.synth_xyz inputs, cleaned as eval/base_model.py:496-498 does.  Only data are written: the
seed and gain (the weights are regenerated from them), the raw f32 xyz input, the float32 fg_logits and center_offsets, the key names
and shapes of the module's state_dict, and two figures about the fixture itself:
    ref_f32_err     max |reference float32 - reference float64| over both outputs
    near_tie_share  share of pixels whose top two float64 logits differ by less than 2e-4
The first (seed, gain) of the search order with ref_f32_err <= 2.5e-5, near_tie_share < 5e-4 and every class on 5-95 % of the frame on
BOTH fixtures is taken, and the conditions are asserted: the GPU test's 1e-4 and its 99.9 % class agreement rest on them."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dsn_torch as D                                    # noqa: E402
from quber_amd import dsn_arch                           # noqa: E402

SIZES = ((96, 128, 31), (48, 80, 32))                    # h, w, scene seed
MAX_F32_ERR, MAX_TIE_SHARE, TIE, FD = 2.5e-5, 5e-4, 2e-4, 64


def reference_networks(ref_dir):
    pkg = types.ModuleType("reference_uois_src")
    pkg.__path__ = [os.path.join(ref_dir, "uois", "src")]
    util = types.ModuleType("reference_uois_src.util")
    util.utilities = types.ModuleType("reference_uois_src.util.utilities")
    sys.modules.update({"reference_uois_src": pkg, "reference_uois_src.util": util, "reference_uois_src.util.utilities": util.utilities})
    spec = importlib.util.spec_from_file_location("reference_uois_src.networks", os.path.join(ref_dir, "uois", "src", "networks.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_uois_src.networks"] = mod
    spec.loader.exec_module(mod)
    return mod


class Net(torch.nn.Module):
    """the attribute names, and with them the state_dict keys, of segmentation.py's DepthSeedingNetwork"""

    def __init__(self, nets):
        super().__init__()
        self.encoder = nets.UNetESP_Encoder(input_channels=3, feature_dim=FD)
        self.decoder = nets.UNetESP_Decoder(feature_dim=FD)
        self.fg_module = torch.nn.Conv2d(FD, 3, kernel_size=1, stride=1, padding=0, bias=False)
        self.cd_module = torch.nn.Conv2d(FD, 3, kernel_size=1, stride=1, padding=0, bias=False)

    def forward(self, xyz):
        f = self.decoder(self.encoder(xyz))
        return self.fg_module(f), self.cd_module(f)


def evaluate(nets, seed, gain):
    sd = dsn_arch.init_state_dict(seed, gain=gain, feature_dim=FD)
    net = Net(nets).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert keys == [(k, tuple(s)) for k, (s, _) in dsn_arch.param_specs(FD).items()], "param_specs differs from the module"
    assert sum(v.numel() for v in net.state_dict().values()) == dsn_arch.N_PARAMS_FD64
    net64 = Net(nets).eval().double()
    net64.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()}, strict=True)
    out = []
    for h, w, scene in SIZES:
        raw = D.synth_xyz(h, w, scene)
        x = D.clean(torch.from_numpy(raw)[None], True)
        with torch.no_grad():
            (l32, o32), (l64, o64) = net(x), net64(x.double())
        err = max(float((l32.double() - l64).abs().max()), float((o32.double() - o64).abs().max()))
        top = torch.sort(l64[0], 0, descending=True).values
        tie = float(((top[0] - top[1]) < TIE).double().mean())
        cls = torch.argmax(l64[0], 0)
        share = [float((cls == k).double().mean()) for k in range(3)]
        out.append(dict(h=h, w=w, scene=scene, xyz=raw, logits=l32[0].numpy(), offsets=o32[0].numpy(), err=err, tie=tie, share=share, keys=keys,
                        span=float(l64.abs().max())))
    return out


def good(r):
    return r["err"] <= MAX_F32_ERR and r["tie"] < MAX_TIE_SHARE and all(0.05 < s < 0.95 for s in r["share"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the directory that holds uois/src/networks.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    nets = reference_networks(a.reference)
    chosen = None
    for gain in (0.7, 0.8, 0.6, 0.5, 1.0):
        for seed in range(8):
            res = evaluate(nets, seed, gain)
            print("seed %d gain %.2f: " % (seed, gain) + "; ".join(
                "%dx%d err %.2e ties %.1e max|logit| %.2f shares %s" % (r["h"], r["w"], r["err"], r["tie"], r["span"], ["%.3f" % s for s in r["share"]])
                for r in res), flush=True)
            if all(good(r) for r in res):
                chosen = (seed, gain, res)
                break
        if chosen:
            break
    assert chosen, "no (seed, gain) of the search order meets the conditions"
    seed, gain, res = chosen
    for r in res:
        assert good(r)
        path = os.path.join(a.out, "dsn_scene_%dx%d.npz" % (r["h"], r["w"]))
        np.savez_compressed(path, seed=np.int64(seed), gain=np.float64(gain), feature_dim=np.int64(FD), scene=np.int64(r["scene"]), xyz=r["xyz"],
                            fg_logits=r["logits"], center_offsets=r["offsets"], keys=np.array([k for k, _ in r["keys"]]),
                            shapes=np.array([list(s) + [0] * (4 - len(s)) for _, s in r["keys"]], np.int32),
                            ref_f32_err=np.float64(r["err"]), near_tie_share=np.float64(r["tie"]), class_shares=np.array(r["share"]))
        size = os.path.getsize(path)
        assert size < 1000000, (path, size)
        print("wrote %s (%d bytes): seed %d gain %.2f ref_f32_err %.3e near_tie_share %.2e" % (path, size, seed, gain, r["err"], r["tie"]))


if __name__ == "__main__":
    main()
