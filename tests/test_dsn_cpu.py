"""CPU: the Depth Seeding Network inventory (quber_amd/dsn_arch.py) and the restatement (tests/dsn_torch.py) against the fixtures
generated from the imported reference module (tests/golden_gen_dsn.py)."""
import os

import numpy as np
import pytest
import torch

import dsn_torch as D
from conftest import golden
from quber_amd import dsn_arch


def _weights(z, dtype=torch.float32):
    sd = dsn_arch.init_state_dict(int(z["seed"]), gain=float(z["gain"]), feature_dim=int(z["feature_dim"]))
    return {k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}


@pytest.mark.parametrize("path", golden("dsn_scene"), ids=os.path.basename)
def test_param_specs_equal_the_module(path):
    z = np.load(path)
    specs = dsn_arch.param_specs(64)
    assert list(specs) == [str(k) for k in z["keys"]]
    assert [tuple(s) for s, _ in specs.values()] == [tuple(int(d) for d in row if d) for row in z["shapes"]]
    assert sum(int(np.prod(s)) for s, _ in specs.values()) == dsn_arch.N_PARAMS_FD64 == 22336768
    for k in ("encoder.layer1.layer1.conv1.weight", "encoder.layer1.layer1.gn1.bias", "encoder.layer3b.dilated16.weight", "encoder.layer3b.gn.weight",
              "decoder.fuse_layer.conv1.weight", "decoder.layer3.channel_reduction_layer.conv1.weight", "decoder.layer3.conv_gn_relu.gn1.weight",
              "decoder.layer5.conv1.weight", "decoder.last_conv.bias", "fg_module.weight", "cd_module.weight"):
        assert k in specs
    # the channel split of the three ESP modules, as the reference computes it
    assert [dsn_arch.esp_split(c) for c in (256, 512, 1024, 20, 64)] == [(51, 52), (102, 104), (204, 208), (4, 4), (12, 16)]
    assert specs["encoder.layer3b.dilated1.weight"][0] == (52, 51, 3, 3) and specs["encoder.layer3b.dilated8.weight"][0] == (51, 51, 3, 3)
    assert specs["decoder.fuse_layer.conv1.weight"][0] == (204, 1024, 1, 1) and specs["encoder.layer4b.conv1.weight"][0] == (102, 512, 3, 3)
    sd = dsn_arch.init_state_dict(3)
    assert list(sd) == list(specs) and all(sd[k].shape == specs[k][0] and sd[k].dtype == np.float32 for k in specs)
    assert float(np.abs(sd["decoder.last_conv.bias"]).max()) > 0 and float(sd["encoder.layer3b.gn.weight"].std()) > 0
    assert np.array_equal(sd["fg_module.weight"], dsn_arch.init_state_dict(3)["fg_module.weight"])
    assert not np.array_equal(sd["fg_module.weight"], dsn_arch.init_state_dict(4)["fg_module.weight"])
    # another feature_dim: the same keys
    assert list(dsn_arch.param_specs(16)) == list(specs) and dsn_arch.param_specs(16)["encoder.layer3b.dilated1.weight"][0] == (16, 12, 3, 3)


@pytest.mark.parametrize("path", golden("dsn_scene"), ids=os.path.basename)
def test_restatement_matches_the_reference(path):
    """float64 restatement against the reference's float32 outputs: |r64 - ref32| <= |r64 - ref64| + |ref64 - ref32| = 0 + ref_f32_err, if the
    restatement is the reference's function (the 1e-9 covers the float64 evaluations' own rounding)."""
    z = np.load(path)
    assert float(z["ref_f32_err"]) <= 2.5e-5 and float(z["near_tie_share"]) < 5e-4          # what the generator asserted
    assert all(0.05 < s < 0.95 for s in z["class_shares"])
    assert np.isnan(z["xyz"]).any()
    x = torch.from_numpy(z["xyz"])[None].double()
    w = _weights(z, torch.float64)
    with torch.no_grad():
        outs = {f: D.forward(x, w, fused=f) for f in (True, False)}
    for f, (lg, off) in outs.items():
        assert lg.shape[1:] == z["fg_logits"].shape == (3,) + z["xyz"].shape[1:]
        for name, got, ref in (("fg_logits", lg, z["fg_logits"]), ("center_offsets", off, z["center_offsets"])):
            err = float((got[0] - torch.from_numpy(ref).double()).abs().max())
            print(f"{os.path.basename(path)} fused {f} {name}: max |restatement f64 - reference f32| {err:.3e}, ref_f32_err {float(z['ref_f32_err']):.3e}")
            assert err <= float(z["ref_f32_err"]) + 1e-9
    # the two plans end in the same tensors (float64: the running sums are added in the same order)
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])


def test_plans_agree_on_every_shared_tap():
    w = {k: torch.from_numpy(v).double() for k, v in dsn_arch.init_state_dict(1, feature_dim=16).items()}
    x = torch.from_numpy(D.synth_xyz(32, 48, 5))[None].double()
    ta, tb = {}, {}
    with torch.no_grad():
        D.forward(x, w, ta, fused=True)
        D.forward(x, w, tb, fused=False)
    shared = sorted((set(ta) & set(tb)) - {"input"})                      # (the raw input holds NaN)
    assert "encoder.layer3b.sum" in shared and "cat1" in shared and "votes" in shared
    for k in shared:
        assert torch.equal(ta[k], tb[k]), k
    assert set(tb) - set(ta) == {f"{n}.dilated{d}" for n in D.ESP for d in dsn_arch.DILATIONS}
    # what the head derives
    assert torch.equal(ta["votes"], ta["xyz"] + ta["center_offsets"])
    assert ta["fg_classes"].dtype == torch.uint8 and torch.equal(ta["fg"], (ta["fg_classes"] == 2).to(torch.uint8))
    assert not torch.isnan(ta["xyz"]).any() and torch.equal(ta["xyz"][:, 1], -torch.nan_to_num(x[:, 1], nan=0.0))
    tc = {}
    D.forward(x, w, tc, negate_y=False)
    assert torch.equal(tc["xyz"][:, 1], torch.nan_to_num(x[:, 1], nan=0.0))


def test_plan_and_ops_lists():
    for fused in (True, False):
        steps, ops = D.plan(fused), D.ops(fused)
        assert len({s.out for s in steps}) == len(steps)                   # every tap is written once
        assert ops == list(dict.fromkeys(s.op for s in steps)) and len(set(ops)) == len(ops)
    # pack; 16 conv + norm pairs, 3 reduce convolutions and ESP norms, 4 pools, 4 upsamplings, last_conv, head; an ESP module's middle is one
    # launch fused and six unfused
    assert len(D.ops(True)) == 1 + 2 * 16 + 2 * 3 + 4 + 4 + 1 + 1 + 3 and len(D.ops(False)) == len(D.ops(True)) + 3 * 5


def test_every_accepted_feature_dim_has_an_esp_kernel():
    """the one-kernel form of an ESP module (option key 53 = 1) has an instance for the split of every module of every feature_dim the
    plan accepts (a multiple of 4 in 8..64): quber_op_esp_kernel is what launch_esp_branches and the plan builder ask.  Host only."""
    from quber_amd import _lib
    lib = _lib.load()
    seen = set()
    for fd in range(8, 65, 4):
        for c in (4 * fd, 8 * fd, 16 * fd):
            n, n1 = dsn_arch.esp_split(c)
            nt = lib.quber_op_esp_kernel(n1)
            assert nt == (n1 + 15) // 16 and 1 <= nt <= 13, (fd, c, n1, nt)
            assert lib.quber_op_esp_packed_floats(n1) == 5 * 9 * nt * nt * 256, (fd, c)
            assert n1 + 4 * n == c and n1 >= n >= 1 and c % fd == 0, (fd, c)
            seen.add(nt)
    assert seen == set(range(1, 14))                                       # every instance belongs to some accepted width
    assert [lib.quber_op_esp_kernel(n1) for n1 in (0, 1, 16, 17, 208, 209, -5)] == [0, 1, 1, 2, 13, 0, 0]
    assert lib.quber_op_esp_packed_floats(0) == 0 and lib.quber_op_esp_packed_floats(209) == 0


def test_first_maximum_wins():
    lg = torch.zeros((1, 3, 1, 4))
    lg[0, :, 0, 0] = torch.tensor([1.0, 2.0, 2.0])                         # a tie of the last two: class 1
    lg[0, :, 0, 1] = torch.tensor([0.5, 0.5, 0.5])                         # all equal: class 0
    lg[0, :, 0, 2] = torch.tensor([0.0, 1.0, 3.0])
    lg[0, :, 0, 3] = torch.tensor([3.0, 1.0, 3.0])                         # first and last: class 0
    assert D.classes(lg).tolist() == [[[1, 0, 2, 0]]]


def test_checkpoint_keys_with_and_without_module_prefix(tmp_path):
    sd = dsn_arch.init_state_dict(2, feature_dim=8)
    plain = dsn_arch.load_checkpoint({"model": {k: torch.from_numpy(v) for k, v in sd.items()}})
    pref = dsn_arch.load_checkpoint({"model": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}})
    bare = dsn_arch.load_checkpoint(dict(sd))
    for got in (plain, pref, bare):
        assert list(got) == list(sd) and all(np.array_equal(got[k], sd[k]) and got[k].dtype == np.float32 for k in sd)
    path = str(tmp_path / "dsn.pth")
    torch.save({"model": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, path)
    disk = dsn_arch.load_checkpoint(path)
    assert list(disk) == list(sd) and all(np.array_equal(disk[k], sd[k]) for k in sd)
    broken = dict(sd)
    del broken["decoder.last_conv.bias"]
    with pytest.raises(KeyError):
        dsn_arch.load_checkpoint(broken)
    wrong = dict(sd)
    wrong["fg_module.weight"] = np.zeros((3, 9, 1, 1), np.float32)
    with pytest.raises(ValueError):
        dsn_arch.load_checkpoint(wrong)
    with pytest.raises(KeyError):
        dsn_arch.load_checkpoint({"model": {"something.else": torch.zeros(1)}})
