"""CPU: every row of the case tables of tests/conv_forms.py takes the route its comment names - kernel, tile shape, K partitions and the place
where the GroupNorm sums are gathered - as the launchers themselves report it (quber_debug_conv_route / _winograd_route / _dual_route: the
launcher walks its own decisions and returns where it would have launched).  Without this a routing change silently turns a gate row of
tests/test_gpu_conv_forms.py into a duplicate of an easy one."""
import pytest

import conv_forms as cf
from quber_amd import _lib


def test_ids_are_unique_and_defaults_cover_every_key():
    ids = [c.id for c in cf.CONV_CASES + cf.ALL_WINO + cf.DUAL_CASES]
    assert len(set(ids)) == len(ids)
    for c in cf.CONV_CASES + cf.ALL_WINO + cf.DUAL_CASES:
        assert set(c.keys) <= set(cf.DEFAULTS), c.id


@pytest.mark.parametrize("c", cf.CONV_CASES, ids=[c.id for c in cf.CONV_CASES])
def test_conv_row_takes_its_route(c):
    r = cf.conv_route(_lib.load(), c)
    assert (r.kernel, r.sums, r.BM, r.BN, r.S, r.tail) == (c.kernel, c.sums, c.BM, c.BN, c.S, c.tail), r


@pytest.mark.parametrize("c", cf.TILE_CASES, ids=[c.id for c in cf.TILE_CASES])
def test_gate_rows_sit_at_the_gate(c):
    """the three gate rows of a tile shape: OH * OW is one tile of rows exactly, one less, one more"""
    oh, ow = cf.out_hw(c)
    for tag, d in (("-at-one-tile-of-rows", 0), ("-one-row-below", -1), ("-one-row-above-tiles-straddle", 1)):
        if c.id.endswith(tag):
            assert oh * ow == c.BM + d
    if "straddle" in c.id or "two-groups" in c.id:
        assert (oh * ow) % c.BM and c.B * oh * ow > 2 * c.BM          # tiles after the first meet two images, the last one is ragged


@pytest.mark.parametrize("c", cf.PERSISTENT_CASES, ids=[c.id for c in cf.PERSISTENT_CASES])
def test_persistent_rows_carry_sums_across_an_image_and_a_group_seam(c):
    """some block of the launch walks, one after the other, tiles of different images and tiles of different groups; in the shared-k rows some
    tile's K is shared between blocks (the fix-up pass gathers its sums), in the others none is"""
    lib = _lib.load()
    r = cf.conv_route(lib, c)
    oh, ow = cf.out_hw(c)
    mtiles, ntiles = -(-c.B * oh * ow // c.BM), -(-c.cout // c.BN)
    assert r.tiles == mtiles * ntiles * c.G and r.min_share > 0
    img = lambda t: ((t % (mtiles * ntiles)) // ntiles * c.BM) // (oh * ow)          # image of a tile's first row
    grp = lambda t: t // (mtiles * ntiles)
    image_seam = group_seam = shared = False
    for walk in cf.persistent_walks(lib, r):
        for (t0, _, _, s0), (t1, _, _, s1) in zip(walk, walk[1:]):
            image_seam |= grp(t0) == grp(t1) and img(t0) != img(t1)
            group_seam |= grp(t0) != grp(t1)
        shared |= any(s >= 0 for _, _, _, s in walk)
    assert image_seam and group_seam and shared == ("shared-k" in c.id), (image_seam, group_seam, shared)


@pytest.mark.parametrize("c", cf.ALL_WINO, ids=[c.id for c in cf.ALL_WINO])
def test_winograd_row_takes_its_route(c):
    r = cf.wino_route(_lib.load(), c)
    assert (r.kernel, r.sums, r.BM, r.S) == (c.kernel, c.sums, c.per_block, c.passes), r
    if c.kernel == "wino":
        assert r.shared_v == int(c.shared and not c.norm)          # one input transform for the heads - not with a norm (its sums are per group)
        assert r.packed == int(c.dil > 1 and c.keys.get(51, 1) == 1 and "dil2" in c.id and r.packed)        # only a dilated row may pack
    for tag, d in (("-at-one-block-of-tiles", 0), ("-one-tile-below", -1)):
        if c.id.endswith(tag):
            assert r.tiles == c.per_block + d, r
    if "one-tile-above" in c.id:
        assert r.tiles > c.per_block and r.tiles % c.per_block, r       # blocks straddle images, the last one is ragged


@pytest.mark.parametrize("c", cf.DUAL_CASES, ids=[c.id for c in cf.DUAL_CASES])
def test_dual_row_takes_its_route(c):
    r = cf.dual_route(_lib.load(), c)
    assert (r.kernel, r.sums, r.BM) == (c.kernel, None, c.BM), r
