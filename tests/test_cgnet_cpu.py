"""CPU: the CGNet inventory and the restatement (tests/cgnet_torch.py) against the fixtures generated from the imported reference
module (tests/golden_gen_cgnet.py), and the two small rules of the UOAIS filter."""
import os

import numpy as np
import pytest
import torch

import cgnet_torch as G
from conftest import golden
from quber_amd import cgnet_arch


def _weights(z, dtype=torch.float32):
    sd = cgnet_arch.init_state_dict(int(z["seed"]), gain=float(z["gain"]))
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


@pytest.mark.parametrize("path", golden("cgnet_scene"), ids=os.path.basename)
def test_param_specs_equal_the_module(path):
    z = np.load(path)
    specs = cgnet_arch.param_specs(classes=2, in_channel=4)
    assert list(specs) == [str(k) for k in z["keys"]]
    assert [tuple(s) for s, _ in specs.values()] == [tuple(int(d) for d in row if d) for row in z["shapes"]]
    for k in ("level1_0.conv.weight", "level2_0.bn.weight", "level2_0.reduce.conv.weight", "level3.7.F_glo.fc.0.bias", "bn_prelu_3.act.weight",
              "classifier.0.conv.weight"):
        assert k in specs
    sd = cgnet_arch.init_state_dict(3)
    assert list(sd) == list(specs) and all(sd[k].shape == specs[k][0] and sd[k].dtype == np.float32 for k in specs)
    # non-trivial statistics, slopes and biases; seeded
    assert float(np.abs(sd["level3.7.F_glo.fc.0.bias"]).max()) > 0 and float(np.abs(sd["b1.bn.running_mean"]).max()) > 0
    assert float(sd["bn_prelu_3.act.weight"].std()) > 0 and float(sd["b1.bn.running_var"].min()) > 0
    assert all(np.array_equal(a, b) for a, b in zip(sd.values(), cgnet_arch.init_state_dict(3).values()))
    assert not np.array_equal(sd["level1_0.conv.weight"], cgnet_arch.init_state_dict(4)["level1_0.conv.weight"])


@pytest.mark.parametrize("path", golden("cgnet_scene"), ids=os.path.basename)
def test_restatement_matches_the_reference(path):
    z = np.load(path)
    assert float(z["ref_f32_err"]) <= 2.5e-5 and float(z["near_tie_share"]) < 5e-4          # what the generator asserted
    x = G.preprocess(z["rgb"], z["depth"])
    w = _weights(z)
    with torch.no_grad():
        fused, unfused = G.forward(x, w, fused=True)[0].numpy(), G.forward(x, w, fused=False)[0].numpy()
    assert fused.shape == z["logits"].shape == (2,) + z["rgb"].shape[:2]
    for name, lg in (("fused", fused), ("unfused", unfused)):
        err = float(np.abs(lg - z["logits"]).max())
        print(f"{os.path.basename(path)} {name}: max |restatement f32 - reference f32| {err:.3e}, 2 x ref_f32_err {2 * float(z['ref_f32_err']):.3e}")
        assert err <= 2 * float(z["ref_f32_err"])
    fg = G.foreground_mask(z["logits"])
    assert fg.dtype == np.uint8 and 0 < fg.mean() < 1


def test_plan_and_ops_lists():
    for fused in (True, False):
        steps, ops = G.plan(fused), G.ops(fused)
        assert len({s.out for s in steps}) == len(steps)                   # every tap is written once
        assert [o for o in ops if not o.endswith(".F_glo.sums")] == list(dict.fromkeys(s.op for s in steps))
    # 22 blocks: two launches each when fused, five when not; the two down blocks are six launches either way
    assert len(G.ops(True)) == 3 + 2 + 2 * 6 + 22 * 2 + 2 + 1 + 3 and len(G.ops(False)) == len(G.ops(True)) + 22 * 3


def test_foreground_mask_first_maximum_wins():
    lg = np.zeros((2, 1, 3), np.float32)
    lg[:, 0, 0] = (1.0, 2.0)
    lg[:, 0, 1] = (2.0, 1.0)
    lg[:, 0, 2] = (1.5, 1.5)                                               # a tie: class 0
    assert G.foreground_mask(lg).tolist() == [[1, 0, 0]]


def test_uoais_filter_rule():
    fg = np.zeros((4, 4), np.uint8)
    fg[:2] = 1
    empty = np.zeros((4, 4), bool)
    half = np.zeros((4, 4), bool)
    half[1:3, 0:2] = True                                                  # 2 of 4 pixels on the foreground: ratio exactly 0.5
    most = np.zeros((4, 4), bool)
    most[0:2, 0:2] = True
    most[2, 0] = True
    most[1, 1] = False                                                     # 3 of 4
    assert (half & fg.astype(bool)).sum() == 2 and half.sum() == 4 and (most & fg.astype(bool)).sum() == 3 and most.sum() == 4
    kept, index = G.uoais_filter([empty, half, most], fg)
    assert index == [2] and len(kept) == 1 and kept[0] is most
    assert G.uoais_filter([], fg) == ([], [])
    # the product's rule on the same counts
    from quber_amd.foreground.predictor import filter_masks_uoais
    counts = np.array([[0, 0], [2, 4], [3, 4]])
    kept2, index2 = filter_masks_uoais([empty, half, most], counts)
    assert index2.tolist() == [2] and kept2[0] is most


def test_upsample_nearest_hand_made():
    img = np.arange(15, dtype=np.uint8).reshape(3, 5)
    up = G.upsample_nearest(img, 6, 10)
    assert up.shape == (6, 10)
    exp = np.repeat(np.repeat(img, 2, axis=0), 2, axis=1)
    assert np.array_equal(up, exp)
    # an odd pair: src = floor(dst * 3 / 4)
    assert G.upsample_nearest(np.arange(3)[None], 1, 4).tolist() == [[0, 0, 1, 2]]
