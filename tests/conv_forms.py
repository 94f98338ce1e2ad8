"""The case tables of tests/test_gpu_conv_forms.py and the host view of the route every row must take (quber_debug_*_route: the launchers'
own decisions, nothing launched).  tests/test_conv_forms_model.py asserts, without a GPU, that each row reaches the path its comment names;
the GPU test asserts it again before it launches.

A row names the option keys it sets (process defaults otherwise), the launch, and the expected route:
  kernel  tile = one tile per block, splitk = ... + splitk_reduce_kernel, persistent, wino = three-kernel pipeline, fused = single Winograd
          kernel, x8 = conv_x8
  sums    where the GroupNorm sums are gathered: the kernel's own name, or sep = a separate pass (launch_gn_stats over the output)"""
import ctypes as C
from collections import namedtuple

KERNEL = {1: "tile", 2: "splitk", 3: "persistent", 4: "wino", 5: "fused", 6: "x8"}
SUMS = {**KERNEL, 0: None, 7: "sep"}
# the process defaults of the keys the rows touch (include/quber_hip.h)
DEFAULTS = {2: 0, 3: 0, 4: 0, 5: 1, 12: 0, 13: 1, 14: 32, 15: 256, 20: 0, 25: 1, 27: 160, 35: 1, 42: 1, 51: 1}
TILE = {1: (64, 64), 2: (128, 128), 3: (128, 64), 4: (256, 32)}
CUS = 256
BCAP_EXTRA = 1          # every slab holds one frame more than the launch's batch

Conv = namedtuple("Conv", "id keys G B H W cin cout k stride pad dil groups affine res relu in_pad out_pad c0 kernel sums BM BN S tail")
Wino = namedtuple("Wino", "id keys G B H W cin cout dil m groups affine relu shared in_place norm norm_groups norm_relu in_pad out_pad c0 kernel sums "
                          "per_block passes")
Dual = namedtuple("Dual", "id keys G B oh ow mid cin stride cout relu kernel BM")


def conv(id, keys, hw, kernel, sums, tile, G=1, B=3, cin=64, cout=128, k=1, stride=1, pad=0, dil=1, groups=32, affine=True, res=False, relu=True,
         in_pad=0, out_pad=0, c0=0, S=1, tail=0):
    return Conv(id, dict(keys), G, B, hw[0], hw[1], cin, cout, k, stride, pad, dil, groups, affine, res, relu, in_pad, out_pad, c0, kernel, sums,
                tile[0], tile[1], S, tail)


def out_hw(c):
    return ((c.H + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1, (c.W + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1)


# ---- one tile per block: per forced tile shape (key 4), 1x1 convolutions of 64 -> 128 channels in 32 norm groups unless the row says otherwise ----
AT = {64: (8, 8), 128: (8, 16), 256: (16, 16)}              # OH * OW = BM exactly
BELOW = {64: (7, 9), 128: (1, 127), 256: (15, 17)}          # BM - 1
ABOVE = {64: (5, 13), 128: (3, 43), 256: (1, 257)}          # BM + 1: every tile after the first meets two images
TILE_CASES = []
for t, (bm, bn) in TILE.items():
    k4, n, at = {4: t, 13: 0}, f"t{bm}x{bn}", AT[bm]
    epi = lambda ohw: "tile" if ohw >= bm else "sep"        # what the rows below that do not sit at the gate expect at this tile shape
    TILE_CASES += [
        conv(f"{n}-at-one-tile-of-rows", k4, at, "tile", "tile", (bm, bn)),
        conv(f"{n}-one-row-below", k4, BELOW[bm], "tile", "sep", (bm, bn)),
        conv(f"{n}-one-row-above-tiles-straddle", k4, ABOVE[bm], "tile", "tile", (bm, bn)),
        conv(f"{n}-cpg2-separate", k4, at, "tile", "sep", (bm, bn), cout=64),
        conv(f"{n}-cpg10-separate", k4, at, "tile", "sep", (bm, bn), cout=320),
        conv(f"{n}-cpg128-column-tiles-share-a-group", k4, at, "tile", "tile", (bm, bn), cout=256, groups=2),
        conv(f"{n}-33-groups-separate", k4, at, "tile", "sep", (bm, bn), cout=132, groups=33),
        conv(f"{n}-scalar-stores-separate", k4, at, "tile", "sep", (bm, bn), out_pad=2),
        conv(f"{n}-3x3-pad1-9x15", k4, (9, 15), "tile", epi(135), (bm, bn), cin=32, k=3, pad=1),
        conv(f"{n}-stride2-17x23-sums-over-9x12", k4, (17, 23), "tile", epi(108), (bm, bn), stride=2),
        conv(f"{n}-residual-relu", k4, ABOVE[bm], "tile", "tile", (bm, bn), res=True),
        conv(f"{n}-no-affine", k4, ABOVE[bm], "tile", "tile", (bm, bn), affine=False, relu=False),
        conv(f"{n}-two-groups-slices", k4, ABOVE[bm], "tile", "tile", (bm, bn), G=2, in_pad=4, out_pad=24, c0=8),
    ]

# ---- split-K: the reduce kernel gathers the sums (keys 2, 3; persistent off).  64 x 64 tiles by launch_conv's own rule ----
SPLITK_CASES = []
for S in (2, 3):
    ks = {2: 1, 3: S, 13: 0}
    for G in (1, 2):
        SPLITK_CASES += [
            conv(f"splitk{S}-g{G}-ohw64", ks, (8, 8), "splitk", "splitk", (64, 64), G=G, cin=256, S=S),
            conv(f"splitk{S}-g{G}-ohw70", ks, (7, 10), "splitk", "splitk", (64, 64), G=G, cin=256, S=S),
        ]
    # 64 channels: a reduce block's 4096 elements are 64 rows + 2 > OH * OW = 64 - the "at most two images per block" cap of the chunk
    SPLITK_CASES.append(conv(f"splitk{S}-chunk-cap-cout64", ks, (8, 8), "splitk", "splitk", (64, 64), cin=256, cout=64, groups=16, S=S))

# the split tail (key 5 = 2: whenever feasible) needs more than a round of 128 x 128 tiles (512) and 32 K-slices: 514 tiles of 1024 input channels.  The
# first 512 tiles gather their own sums in the epilogue, the last two are cut into 4 K-pieces each and the reduce kernel adds theirs (ws_row0 = 65536)
SPLITK_CASES.append(conv("splitk-tail-whole-tiles-and-pieces", {2: 1, 5: 2, 13: 0, 4: 2}, (146, 150), "splitk", "splitk", (128, 128), cin=1024, S=4, tail=2))

# ---- conv_x8 (bf16x3, key 35 = 2: every covered launch): X8_BM = 256 rows ----
X8_CASES = []
for G in (1, 2):
    k8 = {12: 3, 35: 2}
    X8_CASES += [
        conv(f"x8-g{G}-at-one-tile-of-rows", k8, (16, 16), "x8", "x8", (256, 128), G=G, cin=256, cout=256),
        conv(f"x8-g{G}-one-row-below", k8, (15, 17), "x8", "sep", (256, 128), G=G, cin=256, cout=256),
        conv(f"x8-g{G}-three-rows-above", k8, (7, 37), "x8", "x8", (256, 128), G=G, cin=256, cout=256),
    ]

# ---- persistent (keys 2, 13 = 2, 15 = 0, 42 = 0 as test_conv_persistent_vs_torch; key 14 = 1: remainder tiles shared over K), two groups, 128 output
# channels in 32 norm groups.  The smallest OH * OW (found by walking quber_debug_persistent_segments) at which some block's consecutive tiles cross an
# image seam and a group seam: 257 rows per image on 128 x 128 tiles, 86 on 64 x 64.  A share is at least 4 K-slices, so the 128-channel rows (4 slices)
# walk whole tiles only - sums carried from tile to tile in the block - and the 256-channel rows also share remainder tiles over K (sums of the fix-up) ----
PERSISTENT_CASES = []
for dt in (0, 3):
    kp = {2: 1, 13: 2, 14: 1, 15: 0, 42: 0, 12: dt}
    for t, hw in ((2, (1, 257)), (1, (2, 43))):
        bm, bn = TILE[t]
        PERSISTENT_CASES += [
            conv(f"persistent-dt{dt}-t{bm}-whole-tiles", {**kp, 4: t}, hw, "persistent", "persistent", (bm, bn), G=2, cin=128),
            conv(f"persistent-dt{dt}-t{bm}-shared-k", {**kp, 4: t}, hw, "persistent", "persistent", (bm, bn), G=2, cin=256),
        ]


def wino(id, keys, hw, kernel, sums, per_block, G=1, B=3, cin=128, cout=128, dil=1, m=4, groups=32, affine=True, relu=True, shared=False, in_place=False,
         norm=False, norm_groups=32, norm_relu=1, in_pad=0, out_pad=0, c0=0, passes=1):
    return Wino(id, dict(keys), G, B, hw[0], hw[1], cin, cout, dil, m, groups, affine, relu, shared, in_place, norm, norm_groups, norm_relu, in_pad,
                out_pad, c0, kernel, sums, per_block, passes)


# ---- Winograd pipeline (key 25 = 0): 128 -> 128 channels, 32 norm groups.  A block of the output transform takes per_iter * iters tiles: 8 (m = 2, 4:
# 32 lanes per tile) or 4 (m = 6: 64 lanes), iters = 1 at these sizes; the sums are gathered there when an image has at least that many tiles ----
WINO_AT = {2: ((4, 8), (2, 14), (6, 6)), 4: ((8, 16), (4, 28), (12, 12)), 6: ((12, 12), (6, 18), (6, 30))}       # tiles per image: at, one below, one above
WINO_CASES = []
for m, (at, below, above) in WINO_AT.items():
    pb = 4 if m == 6 else 8
    for pack in (0, 1):
        kw = {25: 0, 51: pack}
        WINO_CASES += [
            wino(f"wino-m{m}-pack{pack}-at-one-block-of-tiles", kw, at, "wino", "wino", pb, m=m),
            wino(f"wino-m{m}-pack{pack}-one-tile-below", kw, below, "wino", "sep", pb, m=m),
            wino(f"wino-m{m}-pack{pack}-one-tile-above", kw, above, "wino", "wino", pb, m=m),
            wino(f"wino-m{m}-pack{pack}-dil2-ragged-phases", kw, (9, 13), "wino", "wino", pb, m=m, dil=2),
        ]
    kw = {25: 0}
    WINO_CASES += [
        wino(f"wino-m{m}-two-groups-slices", kw, above, "wino", "wino", pb, m=m, G=2, in_pad=4, out_pad=24, c0=8),
        wino(f"wino-m{m}-three-heads-shared-input", kw, above, "wino", "wino", pb, m=m, G=3, shared=True),
        wino(f"wino-m{m}-three-heads-shared-input-norm", kw, above, "wino", "wino", pb, m=m, G=3, shared=True, norm=True),
        wino(f"wino-m{m}-in-place-norm", kw, above, "wino", "wino", pb, m=m, in_place=True, norm=True),
        wino(f"wino-m{m}-norm-no-relu-two-groups", kw, at, "wino", "wino", pb, m=m, G=2, norm=True, norm_relu=0),
    ]
# key 20 = 1 MiB: 12 tiles of 36 positions x 256 channels are 432 KiB per frame, so the batch of 3 runs in two passes (2 + 1 frames); the sums of the
# second pass must land in image 2
WINO_CASES.append(wino("wino-m4-two-passes", {25: 0, 20: 1}, (12, 16), "wino", "wino", 8, passes=2))

# ---- single Winograd kernel (key 25 = 1, key 27 = 128): blocks of 32 tiles x 32 channels or 16 tiles x 64 channels ----
FUSED_CASES = []
kf = {25: 1, 27: 128}
for name, cin, cout, groups, ft, (at, below, above) in [
        ("c32-64", 32, 64, 16, 16, ((16, 16), (4, 60), (4, 68))),
        ("c64-64", 64, 64, 16, 16, ((16, 16), (4, 60), (4, 68))),
        ("c128-128", 128, 128, 32, 16, ((16, 16), (4, 60), (4, 68))),
        ("c64-32", 64, 32, 8, 32, ((16, 32), (4, 124), (12, 44)))]:
    ng = 32 if cin == 32 else cin // 4        # one channel per norm group of the input (32 channels), else four
    FUSED_CASES += [
        wino(f"fused-{name}-at-one-block-of-tiles", kf, at, "fused", "fused", ft, cin=cin, cout=cout, groups=groups),
        wino(f"fused-{name}-one-tile-below", kf, below, "fused", "sep", ft, cin=cin, cout=cout, groups=groups),
        wino(f"fused-{name}-one-tile-above-two-groups", kf, above, "fused", "fused", ft, cin=cin, cout=cout, groups=groups, G=2, in_pad=4, out_pad=24, c0=8),
        wino(f"fused-{name}-norm-relu-and-sums", kf, above, "fused", "fused", ft, cin=cin, cout=cout, groups=groups, norm=True, norm_groups=ng),
        wino(f"fused-{name}-norm-no-relu", kf, at, "fused", "fused", ft, cin=cin, cout=cout, groups=groups, G=2, norm=True, norm_groups=ng, norm_relu=0),
    ]

# ---- dual 1x1 GEMM: G = 2 (the plan's projection blocks); K = 128 + 160 = 9 slices (bf16x3 keeps its arithmetic above 8), M = 3 * 9 * 13 ragged.
# Persistent (keys 2, 15 = 0) on 64 x 64 tiles at this size, or - bf16x3 with key 35 = 2, stride 1 - conv_x8 ----
DUAL_CASES = []
for dt in (0, 3):
    for stride in (1, 2):
        DUAL_CASES.append(Dual(f"dual-dt{dt}-stride{stride}", {2: 1, 15: 0, 12: dt}, 2, 3, 9, 13, 128, 160, stride, 256, 1, "persistent", 64))
DUAL_CASES.append(Dual("dual-x8-stride1", {2: 1, 15: 0, 12: 3, 35: 2}, 2, 3, 9, 13, 128, 160, 1, 256, 1, "x8", 256))

CONV_CASES = TILE_CASES + SPLITK_CASES + X8_CASES + PERSISTENT_CASES
ALL_WINO = WINO_CASES + FUSED_CASES


class keys_set:
    """the row's option keys for the duration of a block, the defaults afterwards.  Key 2 allocates the 1 GiB split-K workspace of the
    stand-alone ops: only with device=True (the GPU tests); the route queries take `workspace` as an argument instead."""

    def __init__(self, lib, keys, device):
        self.lib, self.keys = lib, {k: v for k, v in keys.items() if device or k != 2}

    def __enter__(self):
        for k, v in self.keys.items():
            self.lib.quber_set_tuning(k, v)

    def __exit__(self, *a):
        for k in self.keys:
            self.lib.quber_set_tuning(k, DEFAULTS[k])


Route = namedtuple("Route", "kernel sums BM BN S tail tiles blocks nk min_share packed shared_v")


def _route(out):
    v = list(out)
    return Route(KERNEL[v[0]], SUMS[v[1]], *v[2:])


def conv_strides(c, Bcap):
    oh, ow = out_hw(c)
    x_cs, y_cs = c.cin + c.in_pad, c.cout + c.out_pad
    return x_cs, Bcap * c.H * c.W * x_cs, y_cs, Bcap * oh * ow * y_cs


def conv_route(lib, c, device=False):
    """the route of quber_op_conv2d_view for row c as tests/test_gpu_conv_forms.py launches it"""
    from quber_amd import _lib
    Bcap = c.B + BCAP_EXTRA
    x_cs, x_gs, y_cs, y_gs = conv_strides(c, Bcap)
    out = (C.c_int32 * 12)()
    with keys_set(lib, c.keys, device):
        _lib.check(lib.quber_debug_conv_route(0, x_cs, x_gs, int(c.affine), 0 if c.res else -1, y_cs, y_gs, c.c0, y_cs, y_gs, c.G, c.B, c.H, c.W, c.cin,
                                              c.cout, c.k, c.stride, c.pad, c.dil, c.groups, c.keys.get(2, 0), CUS, out))
    return _route(out)


def wino_ws_floats(c):
    """workspace of quber_op_conv3x3_winograd_view: V | M of the pipeline for the whole batch, behind the single kernel's filter order"""
    P = (c.m + 2) ** 2
    tiles = c.B * c.dil * c.dil * ((-(-c.H // c.dil) + c.m - 1) // c.m) * ((-(-c.W // c.dil) + c.m - 1) // c.m)
    return c.G * 36 * c.cout * c.cin + c.G * P * tiles * (c.cin + c.cout)


def wino_strides(c, Bcap):
    x_cs, y_cs = c.cin + c.in_pad, c.cout + c.out_pad
    return x_cs, 0 if c.shared else Bcap * c.H * c.W * x_cs, y_cs, Bcap * c.H * c.W * y_cs


def wino_route(lib, c, device=False):
    from quber_amd import _lib
    x_cs, x_gs, y_cs, y_gs = wino_strides(c, c.B + BCAP_EXTRA)
    out = (C.c_int32 * 12)()
    with keys_set(lib, c.keys, device):
        _lib.check(lib.quber_debug_winograd_route(x_cs, x_gs, y_cs, y_gs, int(c.in_place), c.G, c.B, c.H, c.W, c.cin, c.cout, c.dil, c.m, c.groups,
                                                  c.norm_groups if c.norm else 0, wino_ws_floats(c), out))
    return _route(out)


def dual_route(lib, c, device=False):
    from quber_amd import _lib
    h2, w2 = (c.oh - 1) * c.stride + 1, (c.ow - 1) * c.stride + 1
    out = (C.c_int32 * 12)()
    with keys_set(lib, c.keys, device):
        Bcap = c.B + BCAP_EXTRA
        _lib.check(lib.quber_debug_dual_route(Bcap * c.oh * c.ow * c.mid, Bcap * h2 * w2 * c.cin, c.cout * (c.mid + c.cin), c.cout, Bcap * c.oh * c.ow * c.cout,
                                              c.G, c.B, c.oh, c.ow, c.mid, h2, w2, c.cin, c.stride, c.cout, c.keys.get(2, 0), CUS, out))
    return _route(out)


def persistent_walks(lib, r):
    """per block of a persistent launch with route r: its segments (tile, first slice, end slice, slot) - quber_debug_persistent_segments"""
    buf = (C.c_int32 * (4 * 256))()
    walks = []
    for bid in range(r.blocks):
        n = lib.quber_debug_persistent_segments(r.tiles, r.blocks, r.nk, r.min_share, bid, buf, 256)
        walks.append([tuple(buf[4 * i:4 * i + 4]) for i in range(n)])
    return walks
