"""CPU: the host model of the convolution launchers' view-size gates (tests/view_limits.py) and its case table.  Every case of
tests/test_gpu_view_limits.py rests on the arithmetic checked here: the under geometry is taken and the over geometry refused, because of
the one named view; the under view lies within one tap reach of its gate; nothing else keeps the launch from its kernel at 256 CUs."""
import glob
import os
import re

import pytest

import view_limits as vl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the functions that hold a view-size gate, and the row of view_limits.ROWS that restates each
GATE_FUNCTIONS = {"lean_loader": "lean", "conv_persistent_ok": "persistent", "launch_conv_dual": "dual", "launch_conv_x8": "x8", "launch_conv_h8": "h8",
                  "launch_conv_h8p": "h8p", "launch_conv_h8s": "h8s", "winograd_fused_ok": "wino_fused"}

IDS = [c.id for c in vl.CASES]
PAIRS = [c.id for c in vl.CASES if c.over is not None]
SAME_BY_CONSTRUCTION = {"output": ("residual",), "residual": ("output",)}       # a residual has the output's shape


def test_cases_name_every_row_of_the_gate_table():
    assert {c.row for c in vl.CASES} == set(vl.ROWS)
    assert len(set(IDS)) == len(IDS)
    for c in vl.CASES:
        assert c.view in [name for name, _, _ in vl.gate(c.row, c.under, vl.dtype_of(c))] or c.over is None, c.id


def test_every_gate_in_the_sources_has_a_row():
    """The launchers' sources: every function that compares a size with one of the gate constants is one the model restates, with the constant
    the model uses - a launcher that gains a gate shows up here as a function without a row (and then as a row without a case, above)."""
    consts = {r"0x7fffff00L": vl.LIM31, r"\(long\)1 << 31": vl.LIM32, r"\(double\)0x3F000000u": vl.LIMW, r"\(1L << 26\)": vl.REACH}
    assert (0x7fffff00, 1 << 31, 0x3F000000, 1 << 26) == (vl.LIM31, vl.LIM32, vl.LIMW, vl.REACH)
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "quber_amd", "csrc", "*.hip"))):
        fn = None
        for line in open(path):
            m = re.match(r"(?:static )?(?:int|bool) (\w+)\(", line)
            if m:
                fn = m.group(1)
            for pat, value in consts.items():
                if re.search(pat, line) and not line.lstrip().startswith("//"):
                    found.setdefault(fn, set()).add(value)
    assert set(found) == set(GATE_FUNCTIONS), sorted(found)
    assert set(GATE_FUNCTIONS.values()) == set(vl.ROWS)
    for fn, values in found.items():
        row = GATE_FUNCTIONS[fn]
        limits = {lim for dtype in (0, 3) for _, lim, _ in vl.gate(row, vl.CASES[0].under, dtype)}
        assert values <= limits | ({vl.LIM32} if row == "dual" else set()), (fn, values, limits)


@pytest.mark.parametrize("cid", PAIRS)
def test_over_is_under_plus_one_row(cid):
    c = vl.BY_ID[cid]
    field = "W" if c.view == "reach" else "H"           # (the row-reach gate of the single-kernel Winograd form does not depend on H)
    assert c.over == c.under._replace(**{field: getattr(c.under, field) + 1})
    assert c.under.B == 2


@pytest.mark.parametrize("cid", PAIRS)
def test_under_is_taken_and_over_refused_because_of_the_named_view_alone(cid):
    c = vl.BY_ID[cid]
    d = vl.dtype_of(c)
    assert vl.taken(c.row, c.under, d), vl.refusing(c.row, c.under, d)
    assert not vl.taken(c.row, c.over, d)
    same = SAME_BY_CONSTRUCTION.get(c.view, ())
    refusing = vl.refusing(c.row, c.over, d)
    assert c.view in refusing and set(refusing) <= {c.view, *same}, refusing
    # flipping only that view's size (and the view that has its size by construction) flips the verdict, either way
    vu, vo = vl.views(c.under), vl.views(c.over)
    flip = lambda src: {n: src[n] for n in (c.view, *same) if src[n]}
    assert not vl.taken(c.row, c.under, d, override=flip(vo))
    assert vl.taken(c.row, c.over, d, override=flip(vu))
    # every other gated view of the launch: at most half its gate (the over geometry: that plus its one more row)
    for name, lim, _ in vl.gate(c.row, c.under, d):
        if name != c.view and name not in same:
            assert 2 * vu[name] <= lim and vo[name] - vu[name] <= vu[name] // c.under.H, (name, vu[name], vo[name], lim)


@pytest.mark.parametrize("cid", PAIRS)
def test_under_view_is_within_one_tap_reach_of_its_gate(cid):
    c = vl.BY_ID[cid]
    size, (lim, eq) = vl.binding_bytes(c, c.under), vl.limit_of(c, c.under)
    if c.view == "reach":
        assert 0 <= lim - size < c.under.dil * c.under.cin * 24           # one more column crosses
    else:
        assert 0 <= lim - size <= vl.tap_reach_bytes(c, c.under), (size, lim)
    assert vl.passes(size, lim, eq)


def test_the_issue_table_of_binding_views():
    """The arithmetic of the shapes, once more: bytes of the binding view of every under geometry."""
    want = {"A": vl.LIM31 - 256, "B": (1 << 31) - 1024, "C": (1 << 31) - 1024, "D": (1 << 31) - 1024, "Dx": (1 << 31) - 1024, "E": (1 << 31) - 1024,
            "F": vl.LIMW, "F2": vl.LIMW, "H": vl.LIM31 - 256, "I": vl.LIM31 - 256, "J": vl.LIM31 - 256, "K": vl.LIM31 - 256, "K2": vl.LIM31 - 256,
            "L": (1 << 31) - 1024, "M": vl.LIM31 - 256}
    for cid, nbytes in want.items():
        c = vl.BY_ID[cid]
        assert vl.binding_bytes(c, c.under) == nbytes, cid
    f3 = vl.BY_ID["F3"]
    assert f3.under.W == 2912 and vl.views(f3.under)["reach"] <= 1 << 26 < vl.views(f3.over)["reach"]
    # the views that no gate covers: above 2 GiB (H), at 2^32 - 1024 (I), above 2^32 bytes (E2); G: element indices past int
    assert vl.views(vl.BY_ID["H"].under)["output"] > 1 << 31
    assert vl.views(vl.BY_ID["I"].under)["output"] == (1 << 32) - 1024 and vl.views(vl.BY_ID["I"].over)["output"] > 1 << 32
    e2 = vl.views(vl.BY_ID["E2"].under)
    assert e2["output"] > 1 << 32 and e2["residual"] > 1 << 32 and e2["input"] < 1 << 30
    g = vl.BY_ID["G"].under
    assert g.B * g.H * g.W * g.cin > 1 << 31


def test_cases_without_an_over_geometry():
    e2, g = vl.BY_ID["E2"], vl.BY_ID["G"]
    assert vl.taken("x8", e2.under, 3)                                      # no output gate: the launcher takes it
    assert not vl.taken("lean", g.under) and not vl.taken("persistent", g.under)          # above every gate of the fp32 kernels
    assert [c.id for c in vl.CASES if c.over is None] == ["E2", "G"]


@pytest.mark.parametrize("cid", IDS)
def test_nothing_but_the_size_decides_the_route_at_256_cus(cid):
    c = vl.BY_ID[cid]
    for g in (c.under, c.over):
        if g is not None:
            bad = [name for name, ok in vl.preconditions(c, g, 256).items() if not ok]
            assert not bad, (cid, bad)
    assert set(c.keys) <= set(vl.DEFAULTS) and (c.off is None or c.off[0] in vl.DEFAULTS)


@pytest.mark.parametrize("cid", IDS)
def test_device_footprint(cid):
    c = vl.BY_ID[cid]
    cap = vl.FOOTPRINT_GIB.get(cid, 8) * vl.GIB
    for g in (c.under, c.over):
        if g is not None:
            assert vl.footprint(c, g) <= cap, (cid, vl.footprint(c, g) / vl.GIB)
    assert set(vl.FOOTPRINT_GIB) == {"G", "E2", "I"}
