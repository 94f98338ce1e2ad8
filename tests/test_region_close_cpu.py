"""CPU: the scene tests/test_gpu_uois_base.py closes with RegionRefinement(final_close_morphology=True), and what the numpy IMP contract
(tests/test_gms_cpu.py imp_np, largest component off: the loop of uois/src/segmentation.py:556-571 plus the compaction of np.unique) makes of it.

Four instances around a bar, 64 x 112:
  id 1  a bar one row tall: thinner than the 9 x 9 ellipse, the opening removes it, the ids behind it shift down by one
  id 2  two blocks, above the bar on the left and below it on the right
  id 3  two blocks, above the bar on the right and below it on the left: the corners of ids 2 and 3 face each other across the bar, two rows apart
  id 4  a block of its own
The opening rounds the four corners off; once the bar is gone, the closing of id 2 bridges its two corners through the pixels between them, and
so does the closing of id 3 through the same pixels: the later id wins them.  (A bar of two rows or more leaves the rounded corners too far
apart for either closing.)  (A later closing can only ever take what an earlier one ADDED: every pixel an opening keeps lies in an
ellipse inside its own mask, and that ellipse is part of the later id's background.)"""
import numpy as np

from test_gms_cpu import imp_np

H, W, KSIZE = 64, 112, 9


def close_scene():
    ids = np.zeros((H, W), np.int32)
    ids[30:31, 20:104] = 1
    ids[8:30, 30:61] = 2
    ids[31:57, 61:91] = 2
    ids[8:30, 61:91] = 3
    ids[31:57, 30:61] = 3
    ids[40:62, 2:20] = 4
    return ids


def close_np(ids, n_ids, ksize=KSIZE):
    """-> (the map after the final close, compacted; the ids the close removed)"""
    out, report, _ = imp_np(ids, n_ids, ksize, largest=False)
    return out, int(report[1])


def scene_properties(ids, n_ids=4, ksize=KSIZE):
    """asserts (a) and (b) of the module docstring on `ids` -> (the closed map, the pixels the later closing took from the earlier one)"""
    out, removed = close_np(ids, n_ids, ksize)
    assert removed == 1 and out.max() == n_ids - 1, "the bar did not vanish alone"
    assert (out[ids == 1] == 0).any()                                       # some of the bar is background again ...
    for old, new in ((2, 1), (3, 2), (4, 3)):                               # ... and the ids behind it moved down
        core = (ids == old) & (out != 0)
        assert core.any() and (np.bincount(out[core]).argmax() == new), (old, new)
    # what id 2 alone would hold after its own open / close, with id 3 (and 4) left as they are but never processed
    alone, _, _ = imp_np(np.where(ids == 3, 0, ids), n_ids, ksize, largest=False)
    taken = (alone == 1) & (out == 2)
    assert taken.any(), "the closing of the later id took nothing from the earlier one"
    return out, taken


def test_the_scene_has_both_properties():
    ids = close_scene()
    out, taken = scene_properties(ids)
    assert (ids[taken] == 1).any()                                         # contested: the bar's pixels (and corners the openings had rounded off)
    assert out[30, 60] == 2 and out[30, 61] == 2                           # the centre of the bar went to the later id
    # without the close nothing changes: the scene is compact already
    assert sorted(np.unique(ids).tolist()) == [0, 1, 2, 3, 4]
