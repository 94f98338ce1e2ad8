"""Host model of the tile walks of the persistent LDS-DMA convolution kernels (csrc/conv_h8.hip: conv_h8 / h8n / h8p / h8w / h8s kernels;
csrc/conv_x8.hip), shared by tests/test_tile_walks_model.py (CPU) and tests/test_gpu_tile_walks.py (GPU).  A helper, not a test file.

Every kernel gives block (XCD x, j) the tiles start_x + j, + step, ... of its XCD's contiguous run (xcd_runs of test_tile_runs_model.py) and
carries state from one tile of that run into the next: source offsets and filter rows, the next patch, the scale / shift vectors a tile ahead
in rotating LDS images, the GroupNorm partial sums.  What a tile index MEANS differs per kernel family; this file restates it:

    family   pixel tile                      channel tile   tile index                            device code
    h8       256 GEMM rows (b, oy, ox)       256            (g * mtiles + mt) * ntiles + nt       h8_tile_state
    h8n      256 GEMM rows                   one (128)      g * mtiles + mt                       h8_tile_state
    x8       256 GEMM rows                   128            (g * mtiles + mt) * ntiles + nt       x8_tile_state
    h8w      8 x 32 output pixels per image  256            ((g * B + b) * pt + ty * ntx + tx) * ntiles + nt    patch_state
    h8p/h8s  8 x 32 output pixels per image  one            (g * B + b) * pt + ty * ntx + tx      (the kernels' tile lambdas)

The channel tile is the fastest index everywhere.  A GEMM-row tile can straddle two images: its `image` here is the image of its first row."""
from collections import namedtuple

import numpy as np

from test_tile_runs_model import xcd_runs

GATHER = {"h8": 256, "h8n": None, "x8": 128}          # channel-tile width of the 256-row kernels (None: one tile)
PATCH = {"h8w": 256, "h8p": None, "h8s": None}        # ... of the 8 x 32-pixel kernels
ROWS, TY, TX = 256, 8, 32

# a launch as the stand-alone ops take it (fp16: quber_op_conv2d_f16; bf16x3: quber_op_conv2d with key 12 = 3), one group
Case = namedtuple("Case", "id family B H W cin cout k stride pad dil kmode residual relu groups affine")
Step = namedtuple("Step", "tile group image first channel_tile")      # first: first GEMM row (gather) / pixel tile of the image (patch)

TABLE = [
    # id  kernel meant      B    H    W  cin cout  k  s  p  d kmode  res   relu   gn  affine
    Case("A", "h8w", 3, 115, 190, 64, 640, 3, 1, 1, 1, 1, True, True, 0, True),       # one channel block: see launched_family()
    Case("B", "h8w", 3, 115, 190, 128, 640, 3, 1, 1, 1, 1, False, False, 32, True),
    Case("C1", "h8p", 3, 139, 470, 64, 128, 3, 1, 1, 1, 1, True, True, 0, True),
    Case("C2", "h8p", 3, 139, 470, 128, 64, 3, 1, 1, 1, 1, False, False, 16, True),
    Case("D", "h8s", 3, 139, 470, 32, 64, 3, 1, 1, 1, 0, False, True, 0, True),
    Case("E1", "h8", 3, 150, 147, 192, 640, 1, 1, 0, 1, 0, True, True, 0, True),
    Case("E2", "h8", 3, 300, 294, 256, 640, 1, 2, 0, 1, 0, False, False, 0, True),
    Case("F", "h8", 3, 150, 147, 64, 640, 3, 1, 2, 2, 1, False, False, 32, True),
    Case("G", "h8n", 3, 260, 253, 192, 128, 1, 1, 0, 1, 0, False, False, 32, True),
    Case("H", "x8", 3, 150, 147, 288, 384, 1, 1, 0, 1, 0, True, True, 0, True),
    Case("I", "x8", 3, 260, 253, 288, 128, 1, 1, 0, 1, 0, False, False, 0, False),
]
BY_ID = {c.id: c for c in TABLE}


def out_size(c):
    ext = c.dil * (c.k - 1) + 1
    return (c.H + 2 * c.pad - ext) // c.stride + 1, (c.W + 2 * c.pad - ext) // c.stride + 1


def h8w_accepts(cin):
    """launch_conv_h8p's rule for conv_h8w_kernel: at least two 64-channel blocks.  With ONE block the kernel would request the next tile's
    scale / shift vectors at the top of a tile, before any barrier of that tile, into the image that late waves of the previous tile's
    epilogue may still read (two images): such a launch runs on conv_h8_kernel, which rotates three."""
    return cin // 64 >= 2


def launched_family(c, key38=1):
    """The kernel that runs case c: the table's, except where a launcher's gate sends the launch on (h8w with one channel block, key 38 = 2)."""
    if c.family == "h8w" and (key38 == 2 or not h8w_accepts(c.cin)):
        return "h8"
    return c.family


def geometry(c, family=None):
    """-> dict(tiles, ptiles (pixel tiles of the launch), per_image (patch kernels), ntiles (channel tiles), width (channels per tile))."""
    family = family or c.family
    oh, ow = out_size(c)
    if family in GATHER:
        width = GATHER[family] or c.cout
        ptiles, per_image = -(-c.B * oh * ow // ROWS), None
    else:
        assert (oh, ow) == (c.H, c.W), "patch kernels: stride 1, pad 1, 3x3"
        width = PATCH[family] or c.cout
        per_image = -(-oh // TY) * -(-ow // TX)
        ptiles = c.B * per_image
    ntiles = -(-c.cout // width)
    return dict(family=family, tiles=ptiles * ntiles, ptiles=ptiles, per_image=per_image, ntiles=ntiles, width=width, oh=oh, ow=ow)


def step_of(c, geo, tile, groups=1):
    """Tile index -> Step, as the kernels' tile-state code decodes it."""
    tpg = geo["ptiles"] * geo["ntiles"]
    g, rem = divmod(tile, tpg)
    assert g < groups
    pt, nt = divmod(rem, geo["ntiles"])
    if geo["per_image"] is None:
        first = pt * ROWS
        return Step(tile, g, first // (geo["oh"] * geo["ow"]), first, nt)
    b, r2 = divmod(pt, geo["per_image"])
    return Step(tile, g, b, r2, nt)


def walk(c, blocks=256, family=None, groups=1):
    """-> every block's run as a list of Steps (blocks: the device's CU count; fewer tiles than blocks: one block per tile)."""
    geo = geometry(c, family)
    return [[step_of(c, geo, t, groups) for t in run] for run in xcd_runs(groups * geo["tiles"], blocks)]


def _changes(a, b):
    return frozenset(f for f, x, y in (("channel_tile", a.channel_tile, b.channel_tile), ("image", a.image, b.image), ("group", a.group, b.group)) if x != y)


def classify(runs):
    """Counts over all runs.  pairs[f]: consecutive tiles (i, i + 1) of a run that differ in f; triples[f]: tiles (i - 1, i, i + 1) whose OUTER
    two differ in f - what a two-image rotation confuses; f in channel_tile / image / group, plus 'all' (every pair / triple)."""
    pairs = {"all": 0, "channel_tile": 0, "image": 0, "group": 0}
    triples = dict(pairs)
    for run in runs:
        for i in range(len(run) - 1):
            pairs["all"] += 1
            for f in _changes(run[i], run[i + 1]):
                pairs[f] += 1
        for i in range(1, len(run) - 1):
            triples["all"] += 1
            for f in _changes(run[i - 1], run[i + 1]):
                triples[f] += 1
    return dict(pairs=pairs, triples=triples, lengths=sorted({len(r) for r in runs}))


def affine_tiles_at_risk(runs, images, request):
    """The scale / shift image hazard of profiles/r20_h8_affine_race.md for any run.  Tile i's vectors live in image i % images.  The request for
    tile i + 1's vectors is issued during tile i, either at its 'top' (before any barrier of tile i: late waves of tile i - 1's epilogue may
    still read their image) or 'ordered' (behind a barrier every wave passes after tile i - 1's epilogue).  A top request lands in the image of
    tile i + 1 - images; it is a hazard when that is tile i - 1 (images == 2) and the two tiles' vectors differ.  -> sorted tiles at risk."""
    assert request in ("top", "ordered")
    risk = []
    if request == "top" and images == 2:
        for run in runs:
            for i in range(1, len(run) - 1):
                a, b = run[i - 1], run[i + 1]
                if (a.group, a.channel_tile) != (b.group, b.channel_tile):
                    risk.append(a.tile)
    return sorted(risk)


def h8w_request(cin):
    """Where conv_h8w_kernel issues the next tile's vector request: inside its last channel block - the top of the tile when there is only one."""
    return "top" if cin // 64 == 1 else "ordered"


def locate(c, pixel, channel, blocks=256, family=None):
    """Output element (pixel = (b, oy, ox), channel) -> the tile that computes it, its block, its position in that block's run and the run's
    neighbours: dict(tile, block, pos, run (length), step, prev, next) with Steps (None at the ends of a run)."""
    geo = geometry(c, family)
    b, oy, ox = pixel
    if geo["per_image"] is None:
        pt = ((b * geo["oh"] + oy) * geo["ow"] + ox) // ROWS
    else:
        pt = b * geo["per_image"] + (oy // TY) * -(-geo["ow"] // TX) + ox // TX
    tile = pt * geo["ntiles"] + channel // geo["width"]
    for block, run in enumerate(xcd_runs(geo["tiles"], blocks)):
        if tile in run:
            pos = run.index(tile)
            st = lambda t: step_of(c, geo, t)
            return dict(tile=tile, block=block, pos=pos, run=len(run), step=st(tile), prev=st(run[pos - 1]) if pos else None,
                        next=st(run[pos + 1]) if pos + 1 < len(run) else None)
    raise AssertionError(f"tile {tile} is in no run")


def describe(c, pixel, channel, blocks=256, family=None):
    """locate() as one line for an assertion message."""
    w = locate(c, pixel, channel, blocks, family)
    nb = lambda s: "-" if s is None else f"tile {s.tile} (image {s.image}, channel tile {s.channel_tile})"
    return (f"case {c.id} [{family or c.family}] y[{pixel[0]}, {pixel[1]}, {pixel[2]}, {channel}]: tile {w['tile']} (image {w['step'].image}, channel tile "
            f"{w['step'].channel_tile}) = tile {w['pos']} of {w['run']} of block {w['block']}; before it {nb(w['prev'])}, after it {nb(w['next'])}")


# ---- seeded random walks: 3 CUs + 1 ... 5 CUs tiles, 1 / 2 / 3 / 5 channel tiles -------------------------------------------------------------
def random_family(k, cin, cout, dil, key38):
    """The fp16 kernel of a stride-1-or-2 1x1 / padded 3x3 launch with an affine (launch_conv_h8: the patch kernels first)."""
    if k == 3 and dil == 1 and key38:
        if cout <= 128:
            return "h8p"
        if key38 != 2 and h8w_accepts(cin):
            return "h8w"
    return "h8n" if cout == 128 else "h8"


def random_walks(cus, n=12, seed=20253):
    """n fp16 launches as test_gpu_h8.py's fuzz draws them, but of 3 cus + 1 ... 5 cus tiles and 1, 2, 3 or 5 channel tiles -> [(Case, key 38)].
    (seed: the first from 20251 on whose twelve draws at 256 blocks reach all four kernel families and all four channel-tile counts)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        it = len(out)
        k = int(rng.choice([1, 3]))
        cin = int(rng.choice([64, 128, 192])) if k == 3 else int(rng.choice([192, 256, 384]))
        ntn = int(rng.choice([1, 2, 3, 5]))
        cout = int(rng.choice({1: [128], 2: [320, 512], 3: [576, 640, 768], 5: [1088, 1280]}[ntn]))
        dil = int(rng.integers(1, 4)) if k == 3 else 1
        stride = int(rng.choice([1, 2])) if k == 1 else 1
        if stride == 2 and ntn < 3:
            stride = 1                                       # (a strided input of 4 x 3e5 pixels: the launch stays under 1 GB)
        elif stride == 2:
            cin = min(cin, 256)
        B = int(rng.integers(1, 4))
        target = int(rng.integers(3 * cus + 1, 5 * cus + 1))
        residual = bool(rng.random() < 0.3)
        gn = bool(not residual and rng.random() < 0.5)
        relu = bool(rng.random() < 0.5)
        key38 = 1 + it % 2
        family = random_family(k, cin, cout, dil, key38)
        pt = max(1, round(target / ntn))                     # pixel tiles wanted
        if family in GATHER:
            rows = (pt * ROWS - int(rng.integers(0, ROWS))) // B          # output pixels per image
            oh = max(17, int(rows ** 0.5 * rng.uniform(0.6, 1.5)))
            ow = max(17, rows // oh)
        else:
            ntx = int(rng.integers(2, 7))
            nty = max(1, round(pt / (B * ntx)))
            oh, ow = TY * nty - int(rng.integers(0, TY)), TX * ntx - int(rng.integers(0, TX))
        H, W = (oh - 1) * stride + 1 + int(rng.integers(0, stride)), (ow - 1) * stride + 1 + int(rng.integers(0, stride))
        c = Case(f"r{it}", family, B, H, W, cin, cout, k, stride, dil if k == 3 else 0, dil, 1 if k == 3 else 0, residual, relu, 32 if gn else 0, True)
        geo = geometry(c)
        if out_size(c) == (oh, ow) and geo["ntiles"] == (1 if family in ("h8n", "h8p") else ntn) and 3 * cus + 1 <= geo["tiles"] <= 5 * cus:
            out.append((c, key38))
    return out
