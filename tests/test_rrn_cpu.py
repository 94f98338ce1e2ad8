"""CPU: the Region Refinement Network of UOIS-Net-3D - the parameter inventory and the staged restatement (tests/rrn_torch.py) against the
fixtures generated from the imported reference module, and the numpy CONTRACT of the gather / scatter around the network
(rrn_crop_np = rrn_preprocess, rrn_paste_np = rrn_postprocess; csrc/rrn.hip is held to these bit for bit in tests/test_gpu_rrn.py) against
the reference's recorded crops and painted maps (tests/golden/rrn_scene_*.npz, tests/golden_gen_rrn.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rrn_torch as R
from conftest import golden
from quber_amd import dsn_arch, rrn_arch
from test_zoom_cpu import near_index, slot_ok, zoom_rois_np

U = 2.0 ** -24
MAX_ID = 254
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- the contract -----------------------------------------------------------------------------------------------------------------------
def standardize_table_np():
    """standardize_image (eval/preprocess_utils.py:82-93) per byte value: float64, rounded to float32 on assignment; byte channel c takes mean[c]"""
    v = np.arange(256, dtype=np.float64)
    return np.stack([((v / 255. - MEAN[c]) / STD[c]).astype(np.float32) for c in range(3)])


def bilinear_axis(n, S):
    """F.upsample_bilinear (align_corners) from n to S samples in float32 -> (i0, i1, l0, l1)"""
    sc = np.float32(n - 1) / np.float32(S - 1)
    src = np.arange(S, dtype=np.float32) * sc
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = src - i0.astype(np.float32)
    return i0, i1, np.float32(1) - l1, l1


def rrn_crop_np(img, ids, slots, rois, table, S):
    """img u8 [B,H,W,3], ids int [B,H,W], slots int [T,2] = (frame, id), rois i32 [B,n_ids,4], table f32 [3,256] -> (rgb f32 [T,3,S,S],
    mask u8 [T,S,S] of 0 / 1).  Every float32 operation is rounded on its own; a slot that is no crop gives zeros."""
    B, H, W = ids.shape
    T = len(slots)
    rgb, mask = np.zeros((T, 3, S, S), np.float32), np.zeros((T, S, S), np.uint8)
    for t in range(T):
        if not slot_ok(slots[t], rois, B, H, W):
            continue
        f, j = int(slots[t][0]), int(slots[t][1])
        x0, y0, x1, y1 = (int(v) for v in rois[f, j - 1])
        h, w = y1 - y0 + 1, x1 - x0 + 1
        ya, yb, ly0, ly1 = bilinear_axis(h, S)
        xa, xb, lx0, lx1 = bilinear_axis(w, S)
        ly0, ly1 = ly0[:, None], ly1[:, None]
        for c in range(3):
            v = table[c][img[f, y0:y1 + 1, x0:x1 + 1, c]]
            top = lx0 * v[ya][:, xa] + lx1 * v[ya][:, xb]
            bot = lx0 * v[yb][:, xa] + lx1 * v[yb][:, xb]
            rgb[t, c] = ly0 * top + ly1 * bot
            assert rgb.dtype == np.float32 and top.dtype == np.float32
        m = ids[f, y0:y1 + 1, x0:x1 + 1] == j
        mask[t] = m[near_index(S, h)][:, near_index(S, w)]
    return rgb, mask


def rrn_paste_np(refined, slots, rois, z, B, H, W, n_masks):
    """refined u8 [T,S,S], slots int [T,2] ascending by frame, rois i32 [B,n_ids,4], z f32 [B,H,W] -> dict of ids i32 [B,H,W], masks u8
    [B,n_masks,H,W] of 0 / 255, source i32 [B,n_masks], keys f32 [T], report i32 [B,4] = (refined masks, initial masks that vanished, pixels
    painted, pixels painted over)."""
    T = len(slots)
    n_ids = rois.shape[1]
    S = refined.shape[1] if T else 2
    zc = np.where(np.isnan(z), np.float32(0), z)
    keys, cnt, resized = np.zeros(T, np.float32), np.zeros(T, np.int64), [None] * T
    for t in range(T):
        if not slot_ok(slots[t], rois, B, H, W):
            continue
        f, j = int(slots[t][0]), int(slots[t][1])
        x0, y0, x1, y1 = (int(v) for v in rois[f, j - 1])
        m = (refined[t] != 0)[near_index(y1 - y0 + 1, S)][:, near_index(x1 - x0 + 1, S)]
        resized[t] = m
        cnt[t] = int(m.sum())
        if cnt[t]:
            with np.errstate(invalid="ignore"):
                k = np.float32(zc[f, y0:y1 + 1, x0:x1 + 1][m].astype(np.float64).sum() / float(cnt[t]))
            keys[t] = 0 if np.isnan(k) else k                  # both infinities under one mask: no mean, the key reads 0
    out = dict(ids=np.zeros((B, H, W), np.int32), masks=np.zeros((B, n_masks, H, W), np.uint8), source=np.zeros((B, n_masks), np.int32), keys=keys,
               report=np.zeros((B, 4), np.int32))
    for b in range(B):
        mine = [t for t in range(T) if int(slots[t][0]) == b][:MAX_ID]
        order = sorted(mine, key=lambda t: keys[t], reverse=True)                     # stable: equal keys stay in slot order
        owner = np.zeros((H, W), np.int32)
        writes = 0
        for t in order:
            if resized[t] is None or not cnt[t]:
                continue
            j = int(slots[t][1])
            x0, y0, x1, y1 = (int(v) for v in rois[b, j - 1])
            owner[y0:y1 + 1, x0:x1 + 1][resized[t]] = j
            writes += int(cnt[t])
        alive = [j for j in range(1, n_ids + 1) if (owner == j).any()]
        lut = np.zeros(n_ids + 1, np.int32)
        for k, j in enumerate(alive):
            lut[j] = k + 1
            if k < n_masks:
                out["source"][b, k] = j
                out["masks"][b, k] = np.where(owner == j, 255, 0)
        out["ids"][b] = lut[owner]
        gone = sum(1 for t in mine if resized[t] is not None and int(slots[t][1]) not in alive)
        painted = int((owner != 0).sum())
        out["report"][b] = (len(alive), gone, painted, writes - painted)
    return out


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
def load_scene(path):
    """the fixture in the contract's terms: one frame, n_ids = the largest id, one slot per recorded mask id"""
    z = np.load(path)
    ids = z["ids"][None]
    n_ids = int(ids.max())
    slots = np.array([(0, int(m)) for m in z["mask_ids"]], np.int32)
    return z, z["img"][None], ids, n_ids, slots, z["z"][None], int(z["S"])


def contract_cases(h=40, w=56, S=16):
    """the cases the reference cannot record: an empty refined crop, a full crop, a 1 x 1 ROI, equal keys, slots out of range, two frames"""
    rng = np.random.default_rng(9)
    B = 2
    img = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    ids = np.zeros((B, h, w), np.int32)
    ids[0, 4:20, 6:30] = 1
    ids[0, 10:30, 20:50] = 2
    ids[0, h - 1, w - 1] = 3                                                          # a 1 x 1 ROI
    ids[0, 30:38, 2:12] = 5                                                           # id 4 is absent
    ids[1, 5:25, 5:25] = 1
    ids[1, 5:25, 30:50] = 2                                                           # the mirror image of 1 in a constant z: equal keys
    n_ids = 5
    z = (1.0 + 0.3 * rng.random((B, h, w))).astype(np.float32)
    z[1] = 0.75
    z[0, 12, 25] = np.nan
    z[0, 12, 10], z[0, 11, 9] = np.inf, -np.inf                                       # both under slot 0's mask only: no mean, its key reads 0
    rois = zoom_rois_np(ids, n_ids, 0.25)
    slots = np.array([(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 9), (1, 1), (1, 2), (2, 1), (3, 2)], np.int32)       # ascending by frame, as the paste requires; the last two lie behind the batch
    yy, xx = np.mgrid[0:S, 0:S]
    blob = ((yy - S / 2) ** 2 + (xx - S / 2) ** 2 < (S / 2.5) ** 2).astype(np.uint8)
    refined = np.stack([blob] * len(slots))
    refined[1] = 1                                                                    # a full crop: it covers most of mask 1
    refined[4] = 0                                                                    # an empty crop: id 5 vanishes, the ids are compacted
    refined[6:8] = 1                                                                  # overlapping ROIs, equal keys: slot order decides
    return img, ids, n_ids, rois, slots, z, refined, S


@pytest.mark.parametrize("path", golden("rrn_net"), ids=os.path.basename)
def test_inventory_and_restatement_equal_the_reference(path):
    z = np.load(path)
    fd = int(z["feature_dim"])
    specs = rrn_arch.param_specs(fd)
    assert list(specs) == [str(k) for k in z["keys"]]
    assert [tuple(s) for s, _ in specs.values()] == [tuple(int(v) for v in row[:len(s)]) for row, (s, _) in zip(z["shapes"], specs.values())]
    assert sum(int(np.prod(s)) for s, _ in specs.values()) == rrn_arch.N_PARAMS_FD64 == 23070720
    assert float(z["ref_f32_err"]) <= 2.5e-5 and float(z["near_zero_share"]) < 5e-4 and 0.05 < float(z["mask_share"]) < 0.95
    sd = rrn_arch.init_state_dict(int(z["seed"]), gain=float(z["gain"]), feature_dim=fd)
    w = {k: torch.from_numpy(v) for k, v in sd.items()}
    with torch.no_grad():
        got = R.forward(torch.from_numpy(z["rgb"]), torch.from_numpy(z["mask"]), w)
    assert np.array_equal(got.numpy().view(np.uint32), z["logits"].view(np.uint32))
    # the plans of both heads name their ops like the restatement; the checkpoint form loads
    assert R.ops(0)[-2:] == ["decoder.last_conv", "head"] and R.ops(1)[-1] == "head3" and len(R.ops(0)) == len(R.ops(1)) + 1
    ck = {"model": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}
    back = rrn_arch.load_checkpoint(ck)
    assert list(back) == list(specs) and all(np.array_equal(back[k], sd[k]) for k in sd)
    with pytest.raises(KeyError):
        rrn_arch.load_checkpoint(dsn_arch.init_state_dict(0, feature_dim=8))          # the other U-Net's weights


def test_collapsed_head_equals_the_two_layers_in_float64():
    for fd, S in ((8, 12), (64, 9)):
        sd = rrn_arch.init_state_dict(4, feature_dim=fd)
        w64 = {k: torch.from_numpy(v).double() for k, v in sd.items()}
        x = torch.from_numpy(np.random.default_rng(fd).standard_normal((2, fd, S, S)) + 3.0)
        ref = F.conv2d(F.conv2d(x, w64["decoder.last_conv.weight"], w64["decoder.last_conv.bias"], 1, 1), w64["fg_module.weight"])[:, 0]
        got = R.head3(x, w64)
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        w9, b = rrn_arch.collapsed_head(sd)
        w9t, bt = R.collapsed(w64)
        assert np.array_equal(w9, w9t[0].numpy()) and b == float(bt)


def test_threshold():
    assert rrn_arch.logit_threshold(0.5) == 0 and not np.signbit(rrn_arch.logit_threshold(0.5)) and rrn_arch.logit_threshold(0.5).dtype == np.float32
    assert rrn_arch.logit_threshold(0.7) == np.float32(np.log(0.7 / 0.3)) and rrn_arch.logit_threshold(0.25) < 0
    for t in (0.0, 1.0, -1, 2):
        with pytest.raises(ValueError):
            rrn_arch.logit_threshold(t)


@pytest.mark.parametrize("path", golden("rrn_scene"), ids=os.path.basename)
def test_contract_equals_the_reference(path):
    z, img, ids, n_ids, slots, zz, S = load_scene(path)
    assert sorted(set(np.unique(ids)) - {0}) == [int(m) for m in z["mask_ids"]] and n_ids > len(slots), "the fixture's ids have no gap"
    rois = zoom_rois_np(ids, n_ids, float(z["padding"]))
    assert np.array_equal(rois[0][z["mask_ids"] - 1], z["crop_indices"])
    w, h = (z["crop_indices"][:, 2] - z["crop_indices"][:, 0] + 1), (z["crop_indices"][:, 3] - z["crop_indices"][:, 1] + 1)
    assert ((w == 1) & (h == 1)).any() and ((w > S) & (h < S)).any(), "the fixture lost its edge cases"
    rgb, mask = rrn_crop_np(img, ids, slots, rois, standardize_table_np(), S)
    assert np.array_equal(mask, z["mask_crops"])
    for t in range(len(slots)):
        err, bar = float(np.abs(rgb[t] - z["rgb_crops"][t]).max()), 4 * U * float(np.abs(z["rgb_crops"][t]).max())
        print(f"{os.path.basename(path)} crop {t}: max |contract - reference| {err:.3e}, bar {bar:.3e}")
        assert err <= bar
    o = rrn_paste_np(z["refined"], slots, rois, zz, 1, ids.shape[1], ids.shape[2], n_ids)
    k = int(o["report"][0, 0])
    lut = np.concatenate([[0], o["source"][0, :k]])
    assert np.array_equal(lut[o["ids"][0]], z["painted"])                             # the reference keeps the initial ids, np.unique compacts them
    assert np.allclose(o["keys"], z["mean_depths"], rtol=1e-6)
    assert int(o["report"][0, 3]) > 0, "nothing was painted over: the fixture does not show the paint order"
    for i in range(k):
        assert np.array_equal(o["masks"][0, i] == 255, o["ids"][0] == i + 1)
    assert not o["masks"][0, k:].any() and not o["source"][0, k:].any()


def test_contract_cases():
    img, ids, n_ids, rois, slots, z, refined, S = contract_cases()
    B, h, w = ids.shape
    rgb, mask = rrn_crop_np(img, ids, slots, rois, standardize_table_np(), S)
    for t in (3, 5, 8, 9):                                                            # an absent id and slots out of range: zero crops
        assert not rgb[t].any() and not mask[t].any()
    assert mask[2].all() and np.array_equal(rgb[2], np.broadcast_to(standardize_table_np()[np.arange(3), img[0, h - 1, w - 1]][:, None, None], (3, S, S)))
    o = rrn_paste_np(refined, slots, rois, z, B, h, w, n_ids)
    # frame 0: id 5's crop is empty and id 4 has no pixel: three masks survive (1, 2, 3) unless 2's full crop buries 1
    k0 = int(o["report"][0, 0])
    assert list(o["source"][0, :k0]) == sorted(set(np.unique(np.concatenate([[0], o["source"][0, :k0]])[o["ids"][0]])) - {0})
    assert 5 not in o["source"][0] and o["keys"][4] == 0 and int(o["report"][0, 1]) >= 1
    assert set(np.unique(o["ids"][0])) == set(range(k0 + 1))
    assert o["keys"][0] == 0 and np.isfinite(o["keys"]).all() and 1 in o["source"][0]
    # z NaN counts as 0: the key of slot 1 is the float64 mean with that pixel at 0
    x0, y0, x1, y1 = rois[0, 1]
    zc = np.where(np.isnan(z[0]), 0, z[0])[y0:y1 + 1, x0:x1 + 1].astype(np.float64)
    assert o["keys"][1] == np.float32(zc.mean()) and np.isnan(z[0, y0:y1 + 1, x0:x1 + 1]).any()
    # frame 1: equal keys - the later slot is painted last and owns the overlap of the two ROIs
    assert o["keys"][6] == o["keys"][7] == np.float32(0.75)
    ax0, ay0, ax1, ay1 = rois[1, 0]
    bx0, by0, bx1, by1 = rois[1, 1]
    assert ax1 >= bx0, "the ROIs do not overlap"
    assert (o["ids"][1][by0:by1 + 1, bx0:bx1 + 1] == 2).all() and (o["ids"][1][ay0:ay1 + 1, ax0:bx0] == 1).all()
    assert tuple(o["report"][1]) == (2, 0, int((o["ids"][1] != 0).sum()), (ay1 - ay0 + 1) * (ax1 - bx0 + 1))
    # no slots at all
    e = rrn_paste_np(np.zeros((0, S, S), np.uint8), np.zeros((0, 2), np.int32), rois, z, B, h, w, 3)
    assert not e["ids"].any() and not e["masks"].any() and not e["report"].any()
