#!/usr/bin/env python3
"""The route launch_conv / launch_conv_dual take (quber_debug_conv_route, quber_debug_dual_route: the launchers' own decisions, nothing launched, no
GPU needed) for every convolution the refiner sends through them, under the option keys that steer the routing: one line per (launch, key
setting) with the twelve route fields, or the library's refusal.  Two builds of the library route alike when their outputs are equal line for line:
    QUBER_LIB=<other build>/libquber_hip.so python3 tools/route_sweep.py > a.txt;  python3 tools/route_sweep.py > b.txt;  cmp a.txt b.txt
usage: route_sweep.py            (writes to stdout; the last line counts the launches)"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_forms as cf  # noqa: E402
from quber_amd import _lib  # noqa: E402

_argv, sys.argv = sys.argv, sys.argv[:1]        # conv_sweep.py reads its frame count from the command line on import
from conv_sweep import SHAPES  # noqa: E402
sys.argv = _argv

FRAMES = (1, 2, 4, 8, 16)
SIZES = ((480, 640), (720, 1280))
# the process defaults of every key visited (include/quber_hip.h); cf.DEFAULTS has those of the gate rows
DEFAULTS = {**cf.DEFAULTS, 11: 0, 19: 1, 30: 1, 43: 1}
VALUES = {12: (0, 3), 11: (0, 1), 3: (0, 2, 4), 4: (0, 1, 2, 3, 4), 5: (0, 1, 2), 13: (0, 1, 2), 14: (4, 32), 15: (0, 256), 19: (0, 1), 30: (0, 1),
          35: (0, 1, 2), 42: (0, 1, 2), 43: (0, 1)}
PAIRS = ((3, 5), (4, 13), (13, 14, 15), (12, 35), (12, 4))
DILATED_ONLY = (11, 43)             # keys that reach only the dilated 3x3 rows; 43 acts where 11 is set, so those rows take 11 x 43 as well


def settings(dilated):
    """every key against the defaults, plus the cross products of the keys that share a gate: a list of {key: value} without the defaults"""
    groups = [(k,) for k in VALUES if dilated or k not in DILATED_ONLY] + list(PAIRS) + ([DILATED_ONLY] if dilated else [])
    seen = {}
    for g in groups:
        for vals in itertools.product(*(VALUES[k] for k in g)):
            s = {k: v for k, v in zip(g, vals) if v != DEFAULTS[k]}
            seen.setdefault(tuple(sorted(s.items())), s)
    return list(seen.values())


def conv_rows():
    """(label, row, dilated 3x3) of every launch of the table: SHAPES at every frame count and size, and the Winograd position GEMMs of its 3x3 layers"""
    for (fh, fw), F, (name, G, H, W, cin, cout, k, s, d, res) in itertools.product(SIZES, FRAMES, SHAPES):
        H, W = H * fh // 480, W * fw // 640
        for gn, ws in itertools.product((0, 1), (0, 1)):
            if gn and cout % 32:
                continue
            row = cf.conv(name, {2: ws}, (H, W), None, None, (0, 0), G=G, B=F, cin=cin, cout=cout, k=k, stride=s, pad=d * (k // 2), dil=d,
                          groups=32 * gn, res=bool(res))
            yield f"{name} | {fh}x{fw} f{F} G{G} res{res} gn{gn} ws{ws}", row, k == 3 and d > 1
        if k == 3 and s == 1:
            for m, P in ((2, 16), (4, 36)):         # F(m x m, 3x3): P positions = groups of a 1x1 GEMM over the tiles of the batch
                th, tw = d * -(-(-(-H // d)) // m), d * -(-(-(-W // d)) // m)
                row = cf.conv(name, {2: 1}, (th, tw), None, None, (0, 0), G=P, B=G * F, cin=cin, cout=cout, groups=0, affine=False, relu=False)
                yield f"{name} positions m{m} | {fh}x{fw} f{F} G{P} M{G * F * th * tw}", row, False


def dual_rows():
    """conv3 + projection shortcut of the first block of res2 ... res5 as the plan fuses them: two streams, strides as in the table"""
    for (fh, fw), F, (name, oh, ow, mid, cin, stride, cout) in itertools.product(SIZES, FRAMES, (
            ("res2", 120, 160, 64, 64, 1, 256), ("res3", 60, 80, 128, 256, 2, 512), ("res4", 30, 40, 256, 512, 2, 1024), ("res5", 30, 40, 512, 1024, 1, 2048))):
        for ws in (0, 1):
            row = cf.Dual(name, {2: ws}, 2, F, oh * fh // 480, ow * fw // 640, mid, cin, stride, cout, 1, None, 0)
            yield f"{name} conv3 + shortcut | {fh}x{fw} f{F} ws{ws}", row


def visit(lib, route, label, row, setting):
    """one line: the route of `row` under the row's own keys (they win) and `setting`; every key touched is back at its default afterwards"""
    extra = {k: v for k, v in setting.items() if k not in row.keys}
    for k, v in extra.items():
        lib.quber_set_tuning(k, v)
    try:
        r = route(lib, row)
        out = " ".join(str(v) for v in r)
    except _lib.QuberError as e:
        out = f"refused: {e}"
    for k in extra:
        lib.quber_set_tuning(k, DEFAULTS[k])
    print(f"{label} | {' '.join(f'{k}={v}' for k, v in sorted(setting.items())) or 'defaults'} | {out}")


def main():
    lib = _lib.load()
    n = 0
    for label, row, dilated in conv_rows():
        for s in settings(dilated):
            visit(lib, cf.conv_route, label, row, s)
            n += 1
    for label, row in dual_rows():
        for s in settings(False):
            visit(lib, cf.dual_route, label, row, s)
            n += 1
    for c in cf.CONV_CASES:
        for s in settings(c.k == 3 and c.dil > 1):
            visit(lib, cf.conv_route, "gate row " + c.id, c, s)
            n += 1
    for c in cf.DUAL_CASES:
        for s in settings(False):
            visit(lib, cf.dual_route, "gate row " + c.id, c, s)
            n += 1
    print(f"{n} launches")


if __name__ == "__main__":
    main()
