"""CPU: the walk model of tests/tile_walks.py at 256 blocks - the facts that make the launches of tests/test_gpu_tile_walks.py WALK (every block
computes three or four tiles, the channel tile changes on every step of a run where the kernel has channel tiles, runs cross images) - and the
scale / shift image hazard of profiles/r20_h8_affine_race.md extended to a kernel that requests the next tile's vectors at the top of a tile:
conv_h8w_kernel with ONE channel block (Cin = 64), which launch_conv_h8p therefore does not accept (first item)."""
import os
import re

import tile_walks as tw
from test_tile_runs_model import tiles_at_risk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILES = {"A": 810, "B": 810, "C1": 810, "C2": 810, "D": 810, "E1": 777, "E2": 777, "F": 777, "G": 771, "H": 777, "I": 771}


def test_every_table_case_walks_three_or_four_tiles_per_block():
    for c in tw.TABLE:
        geo = tw.geometry(c)
        assert geo["tiles"] == TILES[c.id] and geo["tiles"] >= 769 and geo["tiles"] % 8, c.id
        runs = tw.walk(c)
        assert len(runs) == 256 and sorted(s.tile for r in runs for s in r) == list(range(geo["tiles"])), c.id
        k = tw.classify(runs)
        assert k["lengths"] == [3, 4], (c.id, k["lengths"])
        assert k["pairs"]["all"] == geo["tiles"] - 256 and k["triples"]["all"] == geo["tiles"] - 512, c.id


def test_channel_tile_changes_on_every_step_where_there_are_channel_tiles():
    # three channel tiles, the third ragged on the fp16 kernels; the block step of 32 is no multiple of 3: every pair and every triple changes channel tile
    for ids, pairs, triples in (("AB", 554, 298), (("E1", "E2", "F", "H"), 521, 265)):
        for i in ids:
            c = tw.BY_ID[i]
            geo = tw.geometry(c)
            assert geo["ntiles"] == 3 and (c.cout % geo["width"] or i == "H"), i          # (H: three whole tiles of 128)
            k = tw.classify(tw.walk(c))
            assert k["pairs"]["channel_tile"] == k["pairs"]["all"] == pairs, (i, k)
            assert k["triples"]["channel_tile"] == k["triples"]["all"] == triples, (i, k)


def test_case_a_walks_on_the_gather_kernel_too():
    # one channel block: launch_conv_h8p hands case A to conv_h8_kernel (and key 38 = 2 does the same for any wide layer) - 256-row tiles
    a = tw.BY_ID["A"]
    assert tw.launched_family(a) == "h8" and tw.launched_family(a, key38=2) == "h8"
    assert tw.launched_family(tw.BY_ID["B"]) == "h8w" and tw.launched_family(tw.BY_ID["B"], key38=2) == "h8"
    geo = tw.geometry(a, "h8")
    assert geo["tiles"] == 771 and geo["ntiles"] == 3
    k = tw.classify(tw.walk(a, family="h8"))
    assert k["lengths"] == [3, 4] and k["pairs"]["channel_tile"] == 515 and k["triples"]["channel_tile"] == 259


def test_one_channel_tile_cases_cross_images_inside_runs():
    for i, crossings in (("C1", 64), ("C2", 64), ("D", 64), ("G", 63), ("I", 63)):
        k = tw.classify(tw.walk(tw.BY_ID[i]))
        assert k["pairs"]["channel_tile"] == 0 and k["pairs"]["image"] == crossings, (i, k)


def test_locate_names_the_tile_the_block_and_the_neighbours():
    a = tw.BY_ID["A"]
    for family in ("h8w", "h8"):
        runs = tw.walk(a, family=family)
        for pixel, ch in (((0, 0, 0), 0), ((1, 50, 70), 300), ((2, 114, 189), 639)):
            w = tw.locate(a, pixel, ch, family=family)
            run = runs[w["block"]]
            assert run[w["pos"]] == w["step"] and len(run) == w["run"]
            assert w["prev"] == (run[w["pos"] - 1] if w["pos"] else None)
            assert w["next"] == (run[w["pos"] + 1] if w["pos"] + 1 < len(run) else None)
            assert w["step"].image == pixel[0] and w["step"].channel_tile == ch // 256
            assert f"block {w['block']}" in tw.describe(a, pixel, ch, family=family)
    w = tw.locate(a, (1, 50, 70), 300)          # patch tiling: 15 x 6 tiles per image, three channel tiles
    assert w["tile"] == ((90 + 6 * 6 + 2) * 3 + 1) and w["step"].first == 38
    w = tw.locate(a, (1, 50, 70), 300, family="h8")
    assert w["tile"] == (((115 + 50) * 190 + 70) // 256) * 3 + 1


def test_the_model_restates_the_two_stream_hazard_of_the_gather_kernels():
    # test_tile_runs_model.tiles_at_risk: two images, a request one tile ahead, two streams (groups) in one launch - the measured r20 geometry
    for b, cout in ((9, 512), (12, 512), (14, 512), (9, 128), (14, 128)):
        c = tw.Case("res3", "h8" if cout > 128 else "h8n", b, 60, 80, 128, cout, 1, 1, 0, 1, 0, False, True, 0, True)
        geo = tw.geometry(c)
        got = tw.affine_tiles_at_risk(tw.walk(c, groups=2), 2, "top")
        assert got == tiles_at_risk(geo["ptiles"], geo["ntiles"]), (b, cout)
        assert tw.affine_tiles_at_risk(tw.walk(c, groups=2), 3, "top") == []


def _sweep():
    """Wide undilated 3x3 launches: Cout 256 ... 1024 in steps of 64, 1 - 16 channel blocks, tile counts that give runs of 1 - 5 tiles."""
    for cout in range(256, 1025, 64):
        ntn = -(-cout // 256)
        for cin in (64, 128, 192, 320, 1024):
            for tiles in (97, 256, 300, 520, 777, 810, 1000, 1279):
                nty = -(-tiles // ntn)
                yield tw.Case(f"{cin}>{cout}x{nty}", "h8w", 1, 8 * nty, 32, cin, cout, 3, 1, 1, 1, 1, False, False, 0, True)


def test_a_top_of_tile_request_into_two_images_is_the_r20_hazard():
    a = tw.BY_ID["A"]
    assert tw.h8w_request(a.cin) == "top" and tw.h8w_request(tw.BY_ID["B"].cin) == "ordered"
    risk = tw.affine_tiles_at_risk(tw.walk(a), 2, tw.h8w_request(a.cin))         # conv_h8w_kernel as it would run case A
    assert len(risk) == 298
    assert tw.affine_tiles_at_risk(tw.walk(a), 3, "top") == []                   # a third image (it does not fit: 159 KB of 160)
    assert tw.affine_tiles_at_risk(tw.walk(a), 2, "ordered") == []               # the request behind a barrier
    # without the launcher's rule the sweep is full of them: wherever a run has three tiles and the launch two channel tiles
    unsafe = [c.id for c in _sweep() if tw.affine_tiles_at_risk(tw.walk(c), 2, tw.h8w_request(c.cin))]
    assert unsafe and all(i.startswith("64>") for i in unsafe)
    assert not any(i.startswith("64>256x") for i in unsafe)                      # (one channel tile: every tile of a run has the same vectors)


def test_no_launch_the_wide_patch_kernel_accepts_has_a_tile_at_risk():
    lengths = set()
    for c in _sweep():
        family = tw.launched_family(c)
        runs = tw.walk(c, family=family)
        lengths |= {len(r) for r in runs}
        if family == "h8w":
            assert tw.h8w_accepts(c.cin) and tw.h8w_request(c.cin) == "ordered"
            assert tw.affine_tiles_at_risk(runs, 2, tw.h8w_request(c.cin)) == [], c.id
        else:                                   # conv_h8_kernel: three images, requested at the top of a tile
            assert family == "h8" and c.cin == 64
            assert tw.affine_tiles_at_risk(runs, 3, "top") == [], c.id
    assert lengths >= {1, 2, 3, 4, 5}


def test_the_launcher_states_the_rule_the_model_assumes():
    """tile_walks.h8w_accepts() is launch_conv_h8p's gate and conv_h8w_kernel still has two images and the in-block request: if either side
    changes, this model (and the 298 tiles of case A) has to be looked at again."""
    src = open(os.path.join(ROOT, "quber_amd", "csrc", "conv_h8.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    launcher = code[code.index("int launch_conv_h8p("):code.index("int launch_conv_h8s(")]
    flat = re.sub(r"\s+", "", launcher)
    gate = "if(wide&&p.Kpad/(9*32)<2)return1;"
    assert gate in flat and flat.index(gate) < flat.index("hipLaunchKernelGGL") and flat.index(gate) < flat.index("if(dry)return0;")
    kernel = re.sub(r"\s+", "", code[code.index("void conv_h8w_kernel("):code.index("void conv_h8s_kernel(")])
    assert "smem[SSBASE+2*H8_SS]" in kernel and "issue_ss(ssb^1,gN,n0N)" in kernel and "constintncb=p.Kpad/(9*32);" in kernel


def test_the_random_walks_reach_every_fp16_kernel_and_channel_tile_count():
    draws = tw.random_walks(256)
    assert len(draws) == 12 and draws == tw.random_walks(256)
    assert {c.family for c, _ in draws} == {"h8", "h8n", "h8p", "h8w"}
    assert {tw.geometry(c)["ntiles"] for c, _ in draws} == {1, 2, 3, 5}
    for c, key38 in draws:
        geo = tw.geometry(c)
        assert 3 * 256 + 1 <= geo["tiles"] <= 5 * 256 and {len(r) for r in tw.walk(c)} <= {3, 4, 5}, c
        assert c.family != "h8w" or (key38 == 1 and tw.h8w_accepts(c.cin))
        oh, ow = tw.out_size(c)
        assert (c.B * c.H * c.W * c.cin + (3 + c.residual) * c.B * oh * ow * c.cout) * 2 < 700e6, c          # fp16 input, three outputs alive, residual
