"""A numpy reader for organised ``.pcd`` point clouds (Point Cloud Library file format v0.7), the files the reference reads with
``o3d.io.read_point_cloud`` beside every OCID / OSD / HOPE / DoPose frame (eval/base_model.py:464-479).  ``DATA ascii`` and ``DATA
binary``; ``x y z`` must be ``SIZE 4 TYPE F``, any other field is skipped by its size.  ``DATA binary_compressed`` is not read."""
import numpy as np


def _fail(path, why):
    raise ValueError(f"{path}: {why}")


def read_pcd_xyz(path, h, w):
    """-> f32 [h,w,3], the x, y, z of the h * w points in file order, NaN kept."""
    with open(path, "rb") as f:
        raw = f.read()
    head, pos, data = {}, 0, None
    while data is None:
        end = raw.find(b"\n", pos)
        if end < 0:
            _fail(path, "no DATA line: not a pcd file")
        line = raw[pos:end].decode("ascii", "replace").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, rest = line.partition(" ")
        if key.upper() == "DATA":
            data = rest.strip().lower()
        else:
            head[key.upper()] = rest.split()
    if data not in ("ascii", "binary"):
        _fail(path, f"DATA {data} is not read (ascii and binary are)")
    try:
        fields = head["FIELDS"]
        sizes = [int(v) for v in head["SIZE"]]
        types = [v.upper() for v in head["TYPE"]]
        counts = [int(v) for v in head.get("COUNT", ["1"] * len(fields))]
        width, height = int(head.get("WIDTH", ["0"])[0]), int(head.get("HEIGHT", ["1"])[0])
        points = int(head["POINTS"][0]) if "POINTS" in head else width * height
    except (KeyError, ValueError, IndexError):
        _fail(path, "a header without readable FIELDS / SIZE / TYPE / WIDTH / HEIGHT / POINTS")
    if not (len(fields) == len(sizes) == len(types) == len(counts)):
        _fail(path, "FIELDS, SIZE, TYPE and COUNT name different numbers of fields")
    for name in "xyz":
        if name not in fields:
            _fail(path, f"no field {name!r} among {fields}")
        i = fields.index(name)
        if sizes[i] != 4 or types[i] != "F" or counts[i] != 1:
            _fail(path, f"field {name!r} is SIZE {sizes[i]} TYPE {types[i]} COUNT {counts[i]}, expected 4 F 1")
    if points != h * w or ("WIDTH" in head and width * height != points):
        _fail(path, f"{points} points (WIDTH {width} x HEIGHT {height}) for a frame of {h} x {w} = {h * w}")
    col, offset, at_col, at_byte = 0, 0, {}, {}
    for name, s, c in zip(fields, sizes, counts):
        at_col[name], at_byte[name] = col, offset
        col, offset = col + c, offset + s * c
    if data == "binary":
        if len(raw) - pos < points * offset:
            _fail(path, f"{len(raw) - pos} bytes of data, {points} points of {offset} bytes need {points * offset}")
        rows = np.frombuffer(raw, np.uint8, points * offset, pos).reshape(points, offset)
        out = np.stack([rows[:, at_byte[n]:at_byte[n] + 4].copy().view("<f4")[:, 0] for n in "xyz"], -1)
    else:
        tokens = raw[pos:].split()
        if len(tokens) < points * col:
            _fail(path, f"{len(tokens)} values, {points} points of {col} values need {points * col}")
        rows = np.array(tokens[:points * col]).reshape(points, col)
        try:                                                 # text -> float64 -> float32, the path of a reader that keeps doubles
            out = np.stack([rows[:, at_col[n]].astype(np.float64).astype(np.float32) for n in "xyz"], -1)
        except ValueError:
            _fail(path, "a value of x, y or z that is not a number")
    return np.ascontiguousarray(out.reshape(h, w, 3), dtype=np.float32)
