"""CPU: the device workspace layouts (csrc/common.h WsWalk; the xx_layout function of every file that carves one).

Each layout is stated once in the library, as a walk that hands out the pointers and ends at the total.  The independent second
statement is here: the closed formulas the ``*_ws_bytes`` functions had before the walks replaced them, restated in Python, compared
with ``quber_debug_ws_bytes`` over frames from a single pixel to 480 x 640.  (33, 65) is the smallest frame whose rows are not whole
words, whose planes need padding to 4 words and whose pixel count is no multiple of 16."""
import ctypes
import itertools

import pytest

from quber_amd import _lib

MASK_NMS, COCO_MATCH, SCENE, MEANSHIFT, GMS, ZOOM, LOSSES, CLEANUP, POSTPROCESS = range(9)

FRAMES = ((1, 1), (24, 40), (33, 65), (480, 640))
BATCHES = (1, 3)
COUNTS = (0, 1, 17, 100)
CAPS = (1, 17, 100)              # max_masks of a scene, top_k of the post-processor: at least 1

# sizes the formulas name (csrc): sizeof(InstStat), sizeof(CandList), sizeof(LtCentre); constants of cocoap / meanshift / gms / zoom / losses / cleanup
INST_STAT, CAND_LIST, LT_CENTRE = 48, 8 + 2048 * 8, 32
CA_TOP = 100
MS_SMAX, MS_C, MS_TP, MS_G = 128, 64, 64, 256
GM_SMAX, GM_G, GM_CHUNK = 256, 256, 1024
ZM_MAXID = 254
LS_MAXID, LS_CHUNK, LS_NACC, LS_BINS = 254, 2048, 30, 2048
CC_BINS, SC_CNT, SC_FIN = 256, 8, 8


def al(v):
    return (v + 255) // 256 * 256


def plane_words(h, w):
    return (h * ((w + 31) // 32) + 3) // 4 * 4


def mask_nms(b, n, h, w):
    return al(b * n * plane_words(h, w) * 4) + al((b * n * n + b * n) * 4) + al(b * h * w * 4) + 2 * al(b * n * 4) + al(b * 4)


def coco_match(b, n_gt, h, w, bbox):
    p = CA_TOP + n_gt
    return (0 if bbox else al(b * p * plane_words(h, w) * 4)) + al((b * CA_TOP * n_gt + b * p) * 4) + al(b * p * 4 * 8)


def scene(b, s, m, h, w):
    pw, s = plane_words(h, w), max(s, 1)
    return (al(b * s * pw * 4) + al(b * s * s * 4) + al(b * m * m) + 2 * al(b * m * pw * 4) + al(b * m * 8 * 4) + al(b * m * 4) + al(b * m * 2 * 4) +
            al(b * SC_CNT * 4) + al(b * m * (h + 1) * 4) + al(b * m * (w + 1) * 4) + al(b * m * SC_FIN * 4))


def meanshift(cap_b, h, w):
    n = h * w
    blocks = min((n + MS_TP - 1) // MS_TP, MS_G)
    return 2 * al(cap_b * MS_SMAX * 8) + 2 * al(cap_b * n * 4) + al(cap_b * (MS_SMAX + 1) * 4) + al(cap_b * blocks * MS_SMAX * MS_C * 4)


def gms(cap_b, h, w):
    hw = h * w
    nblk = (hw + GM_CHUNK - 1) // GM_CHUNK
    return (al(cap_b * 16) + 2 * al(cap_b * (GM_SMAX + 1) * 4) + al(cap_b * 64) + al(cap_b * nblk * 4) + al(cap_b * 3 * hw * 4) + 2 * al(cap_b * hw * 4) +
            al(cap_b * GM_G * GM_SMAX * 16))


def zoom(cap_b, h, w):
    tc = cap_b * ZM_MAXID
    keys = tc * (ZM_MAXID + 1)
    return tc * 28 + al(keys * 4) + al(keys) + al(keys * 4) + al(tc * 4) + al(cap_b * 4) + al(cap_b * h * w * 4)


def losses(cap_b, h, w):
    hw = h * w
    nblk = (hw + LS_CHUNK - 1) // LS_CHUNK
    return (al(cap_b * LS_MAXID * 24) + al(cap_b * LS_MAXID * LT_CENTRE) + al(cap_b * nblk * LS_NACC * 8) + al(cap_b * nblk * 8) + al(cap_b * LS_BINS * 4) +
            al(cap_b * 32) + al(cap_b * hw * 8))


def cleanup(b, h, w, cap):
    return 5 * al(b * h * w * 4) + al(b * CC_BINS * 8) + al(b * 255 * 16) + al(b * CC_BINS * 4) + al(b * cap * INST_STAT)


def postprocess(b, h, w, cap):
    hw = h * w
    return al(b * hw * 4) + al(b * hw) + al(b * 256 * 4) * 2 + al(b * cap * INST_STAT) + al(b * CAND_LIST)


@pytest.fixture(scope="module")
def ws_bytes():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.quber_debug_ws_bytes
    fn.restype, fn.argtypes = _lib.SIGNATURES["quber_debug_ws_bytes"]
    return fn


def test_layout_totals_equal_the_closed_formulas(ws_bytes):
    checked = 0
    for (h, w), b in itertools.product(FRAMES, BATCHES):
        for n in COUNTS:
            assert ws_bytes(MASK_NMS, b, n, 0, h, w, 0) == mask_nms(b, n, h, w), ("mask_nms", b, n, h, w)
            for iou_type in (0, 1):
                assert ws_bytes(COCO_MATCH, b, n, 0, h, w, iou_type) == coco_match(b, n, h, w, iou_type), ("coco_match", b, n, h, w, iou_type)
            for m in CAPS:
                assert ws_bytes(SCENE, b, n, m, h, w, 0) == scene(b, n, m, h, w), ("scene", b, n, m, h, w)
            checked += 3 + len(CAPS)
        for cap in CAPS:
            assert ws_bytes(CLEANUP, b, cap, 0, h, w, 0) == cleanup(b, h, w, cap), ("cleanup", b, cap, h, w)
            assert ws_bytes(POSTPROCESS, b, cap, 0, h, w, 0) == postprocess(b, h, w, cap), ("postprocess", b, cap, h, w)
        for which, formula in ((MEANSHIFT, meanshift), (GMS, gms), (ZOOM, zoom), (LOSSES, losses)):
            assert ws_bytes(which, b, 0, 0, h, w, 0) == formula(b, h, w), (formula.__name__, b, h, w)
        checked += 2 * len(CAPS) + 4
    assert checked == len(FRAMES) * len(BATCHES) * (len(COUNTS) * (3 + len(CAPS)) + 2 * len(CAPS) + 4)


def test_caller_allocated_workspaces_equal_the_closed_formulas():
    """The two layouts on the same walk whose size is public: the caller allocates them (quber_eval_batch, quber_inpaint_depth_device)."""
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("quber_eval_batch_workspace_bytes", "quber_inpaint_depth_workspace_bytes"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    lab_max, dnode = 65536, 16
    for (h, w), b in itertools.product(FRAMES, BATCHES):
        px, pp = b * h * w, b * (h + 2) * (w + 2)
        want = al(px) + al(pp) * 4 + al(pp * 4) * 3 + al(pp * 16) + al(pp * dnode) * 2 + al(pp * 4) * 2 + al(64)
        assert lib.quber_inpaint_depth_workspace_bytes(b, h, w) == want, ("inpaint", b, h, w)
        for cap, with_boundary in itertools.product(CAPS, (0, 1)):
            n = b * 2 * lab_max * 4 + 2 * b * cap * cap * 8 + b * 2 * lab_max * 2 + 2 * b * 4
            if with_boundary:
                n += 3 * b * 2 * cap * h * ((w + 63) // 64) * 8
            assert lib.quber_eval_batch_workspace_bytes(b, h, w, cap, with_boundary) == (n + 7) // 8 * 8, ("eval_batch", b, h, w, cap, with_boundary)


def test_unknown_entry(ws_bytes):
    assert ws_bytes(-1, 1, 1, 1, 24, 40, 0) == -1 and ws_bytes(9, 1, 1, 1, 24, 40, 0) == -1
