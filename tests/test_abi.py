"""CPU: the C-ABI library loads and exports every symbol include/quber_hip.h declares; host-side config logic."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from quber_amd import _lib, arch, config


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(quber_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/quber_hip.h but not exported"
    assert set(syms) == set(_lib.SIGNATURES), set(syms) ^ set(_lib.SIGNATURES)


def test_config_struct_matches_header_defaults():
    lib = _lib.load()
    qc = _lib.QuberConfig()
    lib.quber_default_config(ctypes.byref(qc))
    assert (qc.height, qc.width, qc.resnet_depth, qc.top_k, qc.nms_kernel) == (480, 640, 50, 200, 7)
    assert abs(qc.center_threshold - 0.3) < 1e-7 and abs(qc.pixel_mean[5] - 127.5) < 1e-7 and qc.pixel_std[0] == 1.0
    assert b"gfx950" in lib.quber_version()


def test_create_without_gpu_fails_loudly(has_gpu):
    if has_gpu:
        pytest.skip("GPU present")
    lib = _lib.load()
    qc = _lib.QuberConfig()
    lib.quber_default_config(ctypes.byref(qc))
    h = ctypes.c_void_p()
    assert lib.quber_create(ctypes.byref(qc), ctypes.byref(h)) != 0
    assert b"HIP device" in lib.quber_last_error()
    from quber_amd import engine
    with pytest.raises(_lib.QuberError):
        engine.Engine(qc)


def test_yaml_base_merge_and_validation(tmp_path):
    base = tmp_path / "Base.yaml"
    base.write_text("MODEL:\n  META_ARCHITECTURE: MaskRefiner\n  RESNETS:\n    OUT_FEATURES: [res2, res3, res5]\n    RES5_DILATION: 2\n"
                    "  PIXEL_MEAN: [103.53, 116.28, 123.675, 127.5, 127.5, 127.5]\n  PIXEL_STD: [1, 1, 1, 1, 1, 1]\n"
                    "  BACKBONE:\n    FUSION_STRATEGY: add\n    NUM_FUSION_LAYERS: 3\n"
                    "  INS_EMBED_HEAD:\n    NAME: MaskRefinerInsEmbedHead\n    NORM: GN\n    EEE_MASK_ON: True\n    ERROR_TYPE: e2\n"
                    "  PANOPTIC_DEEPLAB:\n    CENTER_THRESHOLD: 0.3\nINPUT:\n  OFFSET_INPUT_ON: True\n  DEPTH_ON: True\nSOLVER:\n  BASE_LR: 0.1\n")
    d = tmp_path / "seed77"
    d.mkdir()
    child = d / "quber.yaml"
    child.write_text("_BASE_: ../Base.yaml\nMODEL:\n  BACKBONE:\n    FUSION_STRATEGY: concat\n    NUM_FUSION_LAYERS: 2\n"
                     "  INS_EMBED_HEAD:\n    HIERARCHICAL_FUSION_ON: True\n    EEE_MASK_ON: False\n"
                     "    HIERARCHY: [[eee_boundary], [foreground, center, offset]]\n    ERROR_TYPE: e3\n")
    cfg = config.merge_from_file(config.get_cfg(), str(child))
    assert cfg.MODEL.BACKBONE.FUSION_STRATEGY == "concat" and cfg.MODEL.BACKBONE.NUM_FUSION_LAYERS == 2
    assert cfg.MODEL.PANOPTIC_DEEPLAB.CENTER_THRESHOLD == 0.3 and cfg.MODEL.PANOPTIC_DEEPLAB.NMS_KERNEL == 7
    assert cfg.SOLVER.BASE_LR == 0.1
    config.validate(cfg)
    # the base file alone (add fusion, flat heads, mask + boundary error heads, e2) is a supported variant too
    flat = config.validate(config.merge_from_file(config.get_cfg(), str(base)))
    kw = config.arch_kwargs(flat)
    assert kw["fusion_add"] and not kw["hierarchical"] and kw["eee_mask_on"] and kw["error_classes"] == 2
    for key, val in (("META_ARCHITECTURE", "PanopticDeepLab"),):
        bad = config.merge_from_file(config.get_cfg(), str(child))
        bad.MODEL[key] = val
        with pytest.raises(config.UnsupportedConfig):
            config.validate(bad)
    bad = config.merge_from_file(config.get_cfg(), str(child))
    bad.MODEL.INS_EMBED_HEAD.HIERARCHY = [["eee_boundary"], ["foreground", "center"]]      # offset head never evaluated
    with pytest.raises(config.UnsupportedConfig):
        config.validate(bad)
    bad = config.merge_from_file(config.get_cfg(), str(child))
    bad.MODEL.SEM_SEG_HEAD.USE_DEPTHWISE_SEPARABLE_CONV = True
    with pytest.raises(config.UnsupportedConfig):
        config.validate(bad)
    config.validate(config.canonical_cfg())


def test_param_specs_match_oracle_module_tree():
    from oracle.network_torch import ArchCfg, MaskRefinerNet
    for depth in (50, 101):
        specs = arch.param_specs(depth=depth)
        sd = MaskRefinerNet(ArchCfg(depth=depth)).state_dict()
        keys = [k for k in sd if not k.endswith("num_batches_tracked")]
        assert set(keys) == set(specs)
        for k in keys:
            assert tuple(sd[k].shape) == tuple(specs[k][0]), k
    assert 79.0e6 < arch.num_parameters() < 80.5e6          # ~79.5 M
    sd = arch.init_state_dict(seed=3)
    sd2 = arch.init_state_dict(seed=3)
    assert all(np.array_equal(sd[k], sd2[k]) for k in sd)


def test_reference_config_zoo_fixture():
    """tests/golden/configs.json (oracle/gen_golden.py configs): what quber_amd/config.py makes of every refiner yaml the
    reference ships.  Asserts (a) the counts the documentation quotes, (b) where the reference's configs/ directory is given
    (QUBER_REFERENCE_CONFIGS) that the reader still derives exactly the stored result from the reference's own files, (c) that every distinct
    architecture the zoo asks for is one the parameter inventory AND the oracle network build, with identical state_dict keys."""
    import json
    import os
    import torch
    from oracle.network_torch import ArchCfg, MaskRefinerNet
    here = os.path.dirname(os.path.abspath(__file__))
    zoo = json.load(open(os.path.join(here, "golden", "configs.json")))
    ok = {k: v for k, v in zoo.items() if "arch" in v}
    assert len(zoo) == 622 and len(ok) == 274
    assert sum("broken" in v for v in zoo.values()) == 223           # _BASE_ files / yaml the reference itself cannot load
    # the evaluation default (eval/run_eval.py:15) and the canonical QuBER config load
    for rel in ("uoais-sim/instance-segmentation/seed77/mask-refiner-rgbd-concat-l2-gn-hf-b-fco-l3-b8.yaml",):
        if rel in zoo:
            assert "arch" in zoo[rel], rel
    sim = {k: v for k, v in zoo.items() if k.startswith("uoais-sim/")}
    assert sum("arch" in v for v in sim.values()) == 134 and sum("unsupported" in v for v in sim.values()) == 0
    # what does not load and is not broken: 124 yamls the reference itself asserts against (RGB-D backbone without DEPTH_ON) and one
    # whose HIERARCHY omits an enabled head, for which the reference raises KeyError at inference (model.py:701-708)
    why = sorted({v["unsupported"][:40] for v in zoo.values() if "unsupported" in v})
    assert len(why) == 2 and sum("unsupported" in v for v in zoo.values()) == 125, why
    root = os.environ.get("QUBER_REFERENCE_CONFIGS")
    if root:
        assert os.path.isdir(root), f"QUBER_REFERENCE_CONFIGS={root} is not a directory"
        for rel, want in zoo.items():
            path = os.path.join(root, rel)
            try:
                cfg = config.validate(config.merge_from_file(config.get_cfg(), path))
            except config.UnsupportedConfig as e:
                assert want == {"unsupported": str(e)}, rel
                continue
            except (FileNotFoundError, __import__("yaml").YAMLError):
                assert "broken" in want, rel
                continue
            kw = config.arch_kwargs(cfg)
            got = dict(kw, hierarchy=[list(l) for l in kw["hierarchy"]], fusion_target=list(kw["fusion_target"]))
            assert want["arch"] == got, rel
            assert want["post"]["center_threshold"] == cfg.MODEL.PANOPTIC_DEEPLAB.CENTER_THRESHOLD
    distinct = {json.dumps(v["arch"], sort_keys=True) for v in ok.values()}
    assert len(distinct) == 87
    for s in sorted(distinct):
        kw = json.loads(s)
        specs = arch.param_specs(**dict(kw, hierarchy=tuple(tuple(l) for l in kw["hierarchy"]), fusion_target=tuple(kw["fusion_target"])))
        with torch.device("meta"):
            net = MaskRefinerNet(ArchCfg(**kw))
        keys = {k for k in net.state_dict() if not k.endswith("num_batches_tracked")}
        assert keys == set(specs), s
