"""Host model of the view-size gates of the convolution launchers, and the table of launches that sit right under and right over each of
them; shared by tests/test_view_limits_model.py (CPU) and tests/test_gpu_view_limits.py (GPU).  A helper, not a test file.

Every fast convolution kernel addresses its operands with 32-bit byte offsets through buffer descriptors; an out-of-range offset constant
supplies the zero padding and drops the rows past the end.  Each launcher therefore refuses views that are too large and hands the launch to a
slower kernel.  This file restates those gates from a launch geometry - which views, their byte sizes AS THE LAUNCHER COMPUTES THEM, the
constant and whether equality passes - and the routing preconditions that are not sizes (option keys, channel multiples, tile counts), so
that a case cannot miss its kernel for another reason:

    row          kernel                                gate (source)                                              falls back to
    lean         exact-fp32 one-tile kernel, LEAN      lean_loader(), conv_igemm.hip: >= 0x7fffff00               per-thread tap arithmetic (64-bit pointers)
    persistent   fp32 / bf16x3 persistent kernel       conv_persistent_ok(), conv_persist.hip: < 1 << 31          one tile per block
    dual         fused conv3 + shortcut                launch_conv_dual(), conv_persist.hip: in2 >= 1 << 31       (stand-alone op: an error)
    x8           bf16x3 LDS-DMA kernel                 launch_conv_x8(), conv_x8.hip: >= 0x7fffff00               conv_igemm.hip
    h8           fp16 gather kernels (h8 / h8n)        launch_conv_h8(), conv_h8.hip: >= 0x7fffff00               128-tile fp16 kernel
    h8p          fp16 patch kernels (h8p / h8w)        launch_conv_h8p(), conv_h8.hip: >= 0x7fffff00              gather kernels
    h8s          fp16 stem kernel                      launch_conv_h8s(), conv_h8.hip: >= 0x7fffff00              128-tile fp16 kernel
    wino_fused   single-kernel Winograd                winograd_fused_ok(), wino_fused.hip: > 0x3F000000,         three-kernel pipeline
                                                       dil * W * cs * 24 > 1 << 26

The fp16 data path hands every K-side quantity over in 4-byte units (launch_conv, conv_igemm.hip: Cin / in_cs / K / Kpad halved), so its input
and weight views come out in bytes when the launchers multiply by 4; outputs and residuals stay in elements of 2 bytes."""
from collections import namedtuple

GIB = 1 << 30
LIM31 = 0x7fffff00          # the LDS-DMA kernels and the LEAN loader: refused when >=
LIM32 = 1 << 31             # conv_persistent_ok(): refused when >=
LIMW = 0x3F000000           # winograd_fused_ok(): refused when >
REACH = 1 << 26             # winograd_fused_ok(): dil * W * cs * 24, refused when >
GUARD_ROWS = 256            # output rows (pixels) of NaN in front of and behind every output: the tallest tile
ROWS = ("lean", "persistent", "dual", "x8", "h8", "h8p", "h8s", "wino_fused")

# the option keys a case may set and their defaults (csrc/common.h: Tuning; 2 / 12: the stand-alone ops, csrc/api_ops.hip)
DEFAULTS = {2: 0, 12: 0, 13: 1, 14: 32, 15: 256, 25: 1, 27: 160, 30: 1, 31: 1, 32: 224, 35: 1, 36: 2, 37: 8, 38: 1, 42: 1}
OP_WS_FLOATS = 256 << 20    # the stand-alone op's split-K workspace (key 2), csrc/api_ops.hip

# a launch as the stand-alone ops take it.  op: conv2d (fp32 / bf16x3: key 12), f16 (quber_op_conv2d_f16), dual (quber_op_conv1x1_dual: `cin`
# channels of the first input, `cin2` of the second, stride 1), wino (quber_op_conv3x3_winograd, m = 4)
Geo = namedtuple("Geo", "op B H W cin cout k stride pad dil kmode residual relu groups affine cin2", defaults=(0,))
# row: the gate table's row; kernel: the kernel meant; view: the one view that crosses; keys: the options of the launch meant; off: the key that sends
# the launch to the other kernel and its value (None: no other kernel); stage / stage_over: the stage profile's names of the two sides;
# over: None for the cases above every gate
Case = namedtuple("Case", "id row kernel view under over keys off stage stage_over note")


def out_size(g):
    ext = g.dil * (g.k - 1) + 1
    return (g.H + 2 * g.pad - ext) // g.stride + 1, (g.W + 2 * g.pad - ext) // g.stride + 1


def es(g):
    return 2 if g.op == "f16" else 4


def kpad(g):
    """Kpad in elements: quber_op_conv2d pads K to 32 floats, quber_op_conv2d_f16 to 64 halfs, the dual op not at all."""
    if g.op == "dual":
        return g.cin + g.cin2
    k = g.k * g.k * g.cin
    return -(-k // 64) * 64 if g.op == "f16" else -(-k // 32) * 32


def views(g):
    """The byte sizes the launchers compare (one group, dense tensors): input, input2, weights, output, residual, planes (the three bf16 weight
    planes of conv_x8.hip), tile (one x8 tile of output rows: out_cs * 256 * 4), and for the Winograd gate win / wout / reach."""
    oh, ow = out_size(g)
    m = g.B * oh * ow
    v = dict(input=g.B * g.H * g.W * g.cin * es(g),                  # fp16: (cin / 2 units) * 4
             weights=g.cout * kpad(g) * es(g),                        # fp16: (Kpad / 2 units) * 4
             output=m * g.cout * es(g), residual=m * g.cout * es(g) if g.residual else 0,
             input2=g.B * g.H * g.W * g.cin2 * 4 if g.op == "dual" else 0,
             planes=3 * g.cout * kpad(g) * 2, tile=g.cout * 256 * 4)
    if g.op == "wino":
        px = g.B * g.H * g.W
        v.update(win=4 * ((px - 1) * g.cin + g.cin), wout=4 * ((px - 1) * g.cout + g.cout), reach=g.dil * g.W * g.cin * 4 * 6)
    return v


def gate(row, g, dtype=0):
    """-> [(view, limit, equality passes)] of the size gate of `row` for this launch.  dtype: key 12 (3: the dual case's x8 path)."""
    if row == "lean":                       # lean_loader(): in_bytes >= 0x7fffff00 || w_bytes >= 0x7fffff00
        return [("input", LIM31, False), ("weights", LIM31, False)]
    if row == "persistent":                 # conv_persistent_ok(): in, out, res, weights < 1 << 31
        return [("input", LIM32, False), ("output", LIM32, False), ("residual", LIM32, False), ("weights", LIM32, False)]
    if row == "dual":
        if dtype == 3:                      # launch_conv_x8(), dual: in2_all, in_all, 3 * plane_bytes >= 0x7fffff00; out_cs * 256 * 4
            return [("input2", LIM31, False), ("input", LIM31, False), ("planes", LIM31, False), ("tile", LIM31, False)]
        # launch_conv_dual(): conv_persistent_ok() and in2_bytes >= 1 << 31
        return [("input2", LIM32, False), ("input", LIM32, False), ("output", LIM32, False), ("weights", LIM32, False)]
    if row == "x8":                         # launch_conv_x8(): in_all, 3 * plane_bytes >= 0x7fffff00, out_cs * X8_BM * 4; NO output gate
        return [("input", LIM31, False), ("planes", LIM31, False), ("tile", LIM31, False)]
    if row == "h8":                         # launch_conv_h8(): in_bytes, w_bytes >= 0x7fffff00; NO output or residual gate
        return [("input", LIM31, False), ("weights", LIM31, False)]
    if row == "h8p":                        # launch_conv_h8p(): in_all, w_all, out_g, res_g (+ n * 8 of the norm coefficients: not in a stand-alone launch)
        return [("input", LIM31, False), ("weights", LIM31, False), ("output", LIM31, False), ("residual", LIM31, False)]
    if row == "h8s":                        # launch_conv_h8s(): in_all, w_all, out_all
        return [("input", LIM31, False), ("weights", LIM31, False), ("output", LIM31, False)]
    if row == "wino_fused":                 # winograd_fused_ok(): in_bytes, out_bytes > 0x3F000000; dil * W * cs * 4 * 6 > 1 << 26
        return [("win", LIMW, True), ("wout", LIMW, True), ("reach", REACH, True)]
    raise KeyError(row)


def passes(size, limit, equal_ok):
    return size <= limit if equal_ok else size < limit


def taken(row, g, dtype=0, override=None):
    """The size gate's verdict.  override: {view: bytes} replaces the sizes of some views."""
    v = dict(views(g), **(override or {}))
    return all(passes(v[name], lim, eq) for name, lim, eq in gate(row, g, dtype))


def refusing(row, g, dtype=0):
    v = views(g)
    return [name for name, lim, eq in gate(row, g, dtype) if not passes(v[name], lim, eq)]


# ---- routing preconditions that are not sizes ---------------------------------------------------------------------------------------------------
def fp32_tile(g, key):
    """launch_conv()'s tile rule (conv_igemm.hip) for the fp32 launches of this table: (BM, BN), or None where the rule would need the split-K
    cost model (launches of under 384 tiles of 128 x 128: none here)."""
    oh, ow = out_size(g)
    m, nk = g.B * oh * ow, kpad(g) // 32
    if g.cout <= 32:
        return 256, 32
    if g.cout <= 64:
        return (128, 64) if (not g.residual and -(-m // 128) >= 1024) else (64, 64)
    if g.residual and nk <= 8 and g.cout >= 128:
        return 64, 64
    tiles128 = -(-m // 128) * -(-g.cout // 128)
    if tiles128 < 384:
        return None
    if key[42] and g.k == 1 and nk >= 16 and tiles128 <= 1280:
        return 64, 64
    if key[42] == 1 and key[12] == 0 and g.k == 1 and nk <= 32:
        return 64, 64
    return 128, 128


def preconditions(c, g, cus=256):
    """-> {name: bool}: everything but the sizes that the launch of case c needs to reach its kernel (the options of c.keys over DEFAULTS)."""
    key = {**DEFAULTS, **c.keys}
    oh, ow = out_size(g)
    m = g.B * oh * ow
    kp, nk = kpad(g), kpad(g) // 32
    p = {}
    if c.row in ("lean", "persistent"):
        tile = fp32_tile(g, key)
        p["fp32 op, not the x8 kernel"] = g.op == "conv2d" and not (key[12] == 3 and g.k == 1 and key[35])
        p["tile rule known"] = tile is not None
    if c.row == "lean":                 # lean_loader(); run<>(): no workspace -> neither persistent nor split
        p["key 30"] = key[30] == 1
        p["Cin % 32, K == Kpad, <= 32 taps"] = g.cin % 32 == 0 and g.k * g.k * g.cin == kp and g.k * g.k <= 32
        p["no workspace"] = key[2] == 0
    if c.row == "persistent":           # run<>() of conv_igemm.hip
        bm, bn = tile
        bpc = 5 if bm == 64 else 2
        tiles = -(-m // bm) * -(-g.cout // bn)
        p["key 13 covers the tile shape"] = (key[13] >= 1 and (bm, bn) == (128, 128)) or (key[13] == 2 and (bm == bn or bm == 256))
        p["BN <= 128, workspace, no skipped rows"] = bn <= 128 and key[2] == 1
        p["16-byte epilogue, one of residual / norm sums"] = g.cout % 4 == 0 and not (g.groups and g.residual)
        p["tiles >= key 15"] = tiles >= key[15]
        p["tiles >= 256 * bpc or K >= key 14"] = tiles >= 256 * bpc or nk >= key[14]
        p["workspace holds 2 * 256 * bpc tiles"] = OP_WS_FLOATS >= 2 * 256 * bpc * bm * bn
    if c.row == "dual":                 # launch_conv_dual(); launch_conv_x8() with a second input
        tiles128 = -(-m // 128) * -(-g.cout // 128)
        p["1x1, stride 1"] = g.k == 1 and g.stride == 1 and g.pad == 0 and g.op == "dual"
        p["K1 % 32, 0 < K1 < K"] = g.cin % 32 == 0 and 0 < g.cin < kp and kp % 32 == 0 and g.cin2 % 4 == 0
        p["keys 13, 2"] = key[13] >= 1 and key[2] == 1
        if key[12] == 3:
            p["key 35 takes every covered launch"] = key[35] == 2 or (key[35] == 1 and nk >= key[37] and g.cout >= 128 and -(-m // 256) * -(-g.cout // 128) >= key[36] * cus)
            p["x8: Cin % 32, two K-slices, 16-byte epilogue"] = g.cin % 32 == 0 and nk >= 2 and g.cout % 4 == 0
        else:
            big = tiles128 >= 192 and g.cout > 64
            p["tiles >= (key 42 ? 2 : 1) * key 15"] = tiles128 >= (2 if key[42] else 1) * key[15]
            p["workspace"] = OP_WS_FLOATS >= 2 * 256 * (2 if big else 5) * (128 * 128 if big else 64 * 64)
            p["16-byte epilogue"] = g.cout % 4 == 0
    if c.row == "x8":                   # launch_conv_x8()
        tiles = -(-m // 256) * -(-g.cout // 128)
        p["keys 12 = 3, 35"] = key[12] == 3 and key[35] >= 1 and g.op == "conv2d"
        p["1x1, pad 0, Cin % 32, K == Kpad, two K-slices"] = g.k == 1 and g.pad == 0 and g.cin % 32 == 0 and nk >= 2
        p["16-byte epilogue"] = g.cout % 4 == 0
        p["keys 36 / 37"] = key[35] == 2 or (nk >= key[37] and g.cout >= 128 and tiles >= key[36] * cus)
    if c.row in ("h8", "h8p", "h8s"):
        cu, ku, kpu = g.cin // 2, g.k * g.k * g.cin // 2, kp // 2           # 4-byte units
        stem = (key[38] and g.k == 3 and g.kmode == 0 and g.stride == 1 and g.pad == 1 and g.dil == 1 and not g.residual and cu == 16 and ku == 144
                and kpu == 160 and g.cout in (32, 64))
        patch = (key[38] and g.k == 3 and g.kmode == 1 and g.stride == 1 and g.pad == 1 and g.dil == 1 and cu % 32 == 0 and ku == kpu and
                 (g.cout in (32, 64, 128) or (g.cout >= 256 and key[38] != 2)))
        ptiles = g.B * -(-g.H // 8) * -(-g.W // 32)
        p["fp16 op, key 31, affine"] = g.op == "f16" and key[31] >= 1 and g.affine
        p["16-byte epilogue"] = g.cout % 8 == 0
    if c.row == "h8s":                  # launch_conv_h8(): the stem shape; launch_conv_h8s()
        p["stem shape"] = bool(stem)
        p["tiles >= key 32"] = ptiles >= key[32]
    if c.row == "h8p":                  # h8_patch_shape(); launch_conv_h8p()
        wide = g.cout > 128
        p["patch shape"] = bool(patch) and not stem
        p["h8w: two channel blocks"] = not wide or kpu // (9 * 32) >= 2
        p["tiles >= key 32"] = ptiles * (-(-g.cout // 256) if wide else 1) >= key[32]
        p["kernel"] = c.kernel == ("conv_h8w_kernel" if wide else "conv_h8p_kernel")
    if c.row == "h8":                   # launch_conv_h8(): neither the stem nor a patch launch; the gather kernels' own conditions
        narrow = g.cout == 128
        p["not a stem / patch launch"] = not stem and not patch
        p["Cin % 64 halfs, K == Kpad, three K-tiles"] = cu % 32 == 0 and ku == kpu and kpu // 32 >= 3
        p["3x3 slice-major or 1x1 pad 0"] = (g.k == 3 and g.kmode == 1) or (g.k == 1 and g.pad == 0)
        p["Cout >= 256 or 128"] = g.cout >= 256 or narrow
        p["tiles >= key 32"] = -(-m // 256) * (1 if narrow else -(-g.cout // 256)) >= key[32]
        p["kernel"] = c.kernel == ("conv_h8n_kernel" if narrow else "conv_h8_kernel")
    if c.row == "wino_fused":           # quber_op_conv3x3_winograd(); winograd_eligible(); winograd_fused_ok()
        p["eligible"] = g.op == "wino" and g.k == 3 and g.stride == 1 and g.pad == g.dil and g.cin % 32 == 0 and g.cin >= 32 and g.cout >= 32
        p["key 25, exact fp32"] = key[25] == 1 and key[12] in (0, 3)
        p["32 | Cout, Cin <= key 27"] = g.cout % 32 == 0 and g.cin <= key[27]
    return p


def wino_tiles(g):
    """Tiles of the three-kernel F(4x4) pipeline, one tiling per dilation phase (its workspace holds 36 * tiles * (Cin + Cout) floats)."""
    ceil = lambda a, b: -(-a // b)
    return g.B * g.dil * g.dil * ceil(ceil(g.H, g.dil), 4) * ceil(ceil(g.W, g.dil), 4)


def footprint(c, g):
    """Device bytes the GPU test of this launch holds at its peak: operands, the output (and the other kernel's) with their guards, the residual,
    the Winograd workspace, the stand-alone op's split-K workspace where key 2 is set."""
    v = views(g)
    oh, ow = out_size(g)
    outs = 2 if (c.off or c.row == "dual") else 1
    n = v["input"] + v["input2"] + v["weights"] * 2 + v["residual"] + outs * (v["output"] + 2 * GUARD_ROWS * g.cout * es(g))
    if g.op == "wino":
        n += 4 * (36 * wino_tiles(g) * (g.cin + g.cout) + 2 * 36 * g.cout * g.cin)
    if c.keys.get(2):
        n += 4 * OP_WS_FLOATS
    if c.keys.get(12) == 3 or c.row == "dual":
        n += v["planes"]
    return n


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def _pair(g):
    return g, g._replace(H=g.H + 1)


def _g(op, B, H, W, cin, cout, k=1, pad=0, dil=1, kmode=0, residual=False, relu=True, groups=0, cin2=0):
    return Geo(op, B, H, W, cin, cout, k, 1, pad, dil, kmode, residual, relu, groups, True, cin2)


_F3 = _g("wino", 2, 40, (1 << 26) // (6 * 160 * 24), 160, 32, 3, 6, 6)

CASES = [
    Case("A", "lean", "conv_igemm_f32 LEAN", "input", *_pair(_g("conv2d", 2, 2049, 2047, 64, 32, 3, 2, 2, 1)), {}, (30, 0), "conv_gemm", "conv_gemm",
         "a padding tap of the first pixel reaches at most (pad rows + pad columns) before the view: offsets stay inside int32"),
    Case("B", "persistent", "conv_igemm_pk 256x32", "input", *_pair(_g("conv2d", 2, 889, 2359, 128, 32, 3, 2, 2, 1)), {2: 1, 13: 2, 15: 0, 42: 0}, (13, 0),
         "conv_gemm", "conv_gemm", "every view below 2 GiB: OOB = 0x80000000 is past the range, a wrapped window origin + off comes back inside"),
    Case("C", "persistent", "conv_igemm_pk 128x128", "output", *_pair(_g("conv2d", 2, 889, 2359, 32, 128, 3, 1, 1, 1, residual=True)), {2: 1}, (13, 0),
         "conv_gemm", "conv_gemm", "the output descriptor of a tile ends at the end of the tensor, which drops the rows past M of the last m-tile"),
    Case("D", "dual", "conv_igemm_pk dual 64x64", "input2", *_pair(_g("dual", 2, 889, 2359, 64, 64, cin2=128)), {2: 1}, None, "conv_gemm", None,
         "in2_bytes >= 1 << 31 is refused; OOB for the rows past M"),
    Case("Dx", "dual", "conv_x8_kernel dual", "input2", *_pair(_g("dual", 2, 889, 2359, 64, 64, cin2=128)), {2: 1, 12: 3, 35: 2}, None, "conv_gemm_x8", None,
         "descriptor range of the second input (ws_rows): in2_all < 0x7fffff00"),
    Case("E", "x8", "conv_x8_kernel", "input", *_pair(_g("conv2d", 2, 889, 2359, 128, 128)), {12: 3, 35: 2}, (35, 0), "conv_gemm_x8", "conv_gemm",
         "X8_OOB past every descriptor range; per-tile output descriptors from a 64-bit origin"),
    Case("E2", "x8", "conv_x8_kernel", "output", _g("conv2d", 2, 1400, 1023, 64, 384, residual=True), None, {12: 3, 35: 2}, (35, 0), "conv_gemm_x8", None,
         "no output gate: per-tile output / residual descriptors from a 64-bit origin, out_cs * 256 * 4 inside a descriptor"),
    Case("F", "wino_fused", "wino_fused_kernel", "win", *_pair(_g("wino", 2, 1344, 1536, 64, 32, 3, 1, 1)), {25: 1}, (25, 0), "wino_fused", "wino_input",
         "OOBH = 0x40000000 once per invalid row and once per invalid column: past any view of at most 0x3F000000 bytes"),
    Case("F2", "wino_fused", "wino_fused_kernel", "wout", *_pair(_g("wino", 2, 1344, 1536, 32, 64, 3, 1, 1)), {25: 1}, (25, 0), "wino_fused", "wino_input",
         "the output rows and columns past the image carry OOBH: dropped by the range check"),
    Case("F3", "wino_fused", "wino_fused_kernel", "reach", _F3, _F3._replace(W=_F3.W + 1), {25: 1}, (25, 0), "wino_fused", "wino_input",
         "five dilated rows of a window stay inside 1 << 26 bytes, so row and column terms never reach OOBH"),
    Case("H", "h8", "conv_h8_kernel", "input", *_pair(_g("f16", 2, 1366, 2047, 192, 256)), {}, (31, 0), "conv_gemm_h8", "conv_gemm",
         "H8_OOB past every descriptor range (+ 32 rows: still past every range); no output gate: per-tile descriptors, 64-bit tile origin"),
    Case("I", "h8", "conv_h8_kernel", "input", *_pair(_g("f16", 2, 2049, 2047, 128, 256, 3, 2, 2, 1)), {}, (31, 0), "conv_gemm_h8", "conv_gemm",
         "the dilated taps of the DMA gather; an output of 2^32 - 1024 bytes behind per-tile descriptors"),
    Case("J", "h8", "conv_h8n_kernel", "input", *_pair(_g("f16", 2, 1366, 2047, 192, 128, relu=False, groups=32)), {}, (31, 0), "conv_gemm_h8", "conv_gemm",
         "the narrow gather kernel's descriptors and its norm sums at the last tile"),
    Case("K", "h8p", "conv_h8p_kernel", "input", *_pair(_g("f16", 2, 2049, 2047, 128, 64, 3, 1, 1, 1)), {}, (38, 0), "conv_gemm_h8", "conv_gemm",
         "patch rows past the image are requested at H8_OOB: zeros"),
    Case("K2", "h8p", "conv_h8p_kernel", "output", *_pair(_g("f16", 2, 2049, 2047, 64, 128, 3, 1, 1, 1, residual=True)), {}, (38, 0), "conv_gemm_h8", "conv_gemm_h8",
         "descriptor ranges of one group's output / residual view (pk_min / pk_in2_bytes) as int"),
    Case("L", "h8p", "conv_h8w_kernel", "output", *_pair(_g("f16", 2, 889, 2359, 128, 256, 3, 1, 1, 1, relu=False, groups=32)), {}, (38, 2), "conv_gemm_h8", "conv_gemm_h8",
         "the wide patch kernel's output view and its norm sums"),
    Case("M", "h8s", "conv_h8s_kernel", "output", *_pair(_g("f16", 2, 4098, 2047, 32, 64, 3, 1, 1, 0)), {}, (38, 0), "conv_gemm_h8", "conv_gemm",
         "the stem kernel's one output descriptor over all groups"),
    Case("G", "lean", "conv_igemm_f32 (pointers)", "input", _g("conv2d", 2, 4097, 4096, 64, 16), None, {}, None, "conv_gemm", None,
         "element indices past int: the one-tile kernel's 64-bit pointer arithmetic"),
]
BY_ID = {c.id: c for c in CASES}
# E2 and I cannot meet 8 GiB: an output above 2^32 bytes with a residual of the same size (E2), or twice - the kernel's and the other kernel's - next
# to a 2 GiB input (I)
FOOTPRINT_GIB = {"G": 12, "E2": 14, "I": 11}


def dtype_of(c):
    return c.keys.get(12, 0)


def binding_bytes(c, g):
    return views(g)[c.view]


def tap_reach_bytes(c, g):
    """One tap reach - dil * (W + 1) pixels - of the binding view, in its bytes."""
    per_pixel = {"input": g.cin * es(g), "input2": g.cin2 * 4, "output": g.cout * es(g), "win": g.cin * 4, "wout": g.cout * 4}[c.view]
    return g.dil * (g.W + 1) * per_pixel


def limit_of(c, g):
    return next((lim, eq) for name, lim, eq in gate(c.row, g, dtype_of(c)) if name == c.view)
