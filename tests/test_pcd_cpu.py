"""CPU: quber_amd.pcd.read_pcd_xyz on files the test writes itself - ascii and binary, 3 x 5, an extra rgb field before and after x y z,
NaN rows, and the three refusals (binary_compressed, a point count that does not match, a missing field)."""
import numpy as np
import pytest

from quber_amd.pcd import read_pcd_xyz

H, W = 3, 5


def points(seed=0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-2.0, 2.0, (H * W, 3)).astype(np.float32)
    xyz[4] = np.nan                                                    # a whole NaN row: a pixel without depth
    xyz[9, 1] = np.nan
    xyz[2] = (0.0, -0.0, 1e-42)
    return xyz


def write_pcd(path, xyz, data="ascii", layout=("x", "y", "z"), width=W, height=H, n_points=None, viewpoint=True):
    """layout: field names in file order; 'rgb' is one 4-byte float (PCL's packed colour), 'label' one 2-byte unsigned"""
    n = len(xyz)
    rng = np.random.default_rng(7)
    cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "rgb": rng.uniform(1e5, 4e6, n).astype(np.float32),
            "label": rng.integers(0, 600, n).astype(np.uint16), "normal": rng.uniform(-1, 1, (n, 3)).astype(np.float32)}
    size = {"x": 4, "y": 4, "z": 4, "rgb": 4, "label": 2, "normal": 4}
    typ = {"x": "F", "y": "F", "z": "F", "rgb": "F", "label": "U", "normal": "F"}
    cnt = {k: (3 if k == "normal" else 1) for k in size}
    head = ["# .PCD v0.7 - Point Cloud Data file format", "VERSION 0.7", "FIELDS " + " ".join(layout), "SIZE " + " ".join(str(size[f]) for f in layout),
            "TYPE " + " ".join(typ[f] for f in layout), "COUNT " + " ".join(str(cnt[f]) for f in layout), "WIDTH %d" % width, "HEIGHT %d" % height]
    if viewpoint:
        head.append("VIEWPOINT 0 0 0 1 0 0 0")
    head += ["POINTS %d" % (n if n_points is None else n_points), "DATA " + data]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if data == "ascii":
            for i in range(n):
                vals = []
                for name in layout:
                    v = np.atleast_1d(cols[name][i])
                    vals += [repr(float(q)) if typ[name] == "F" else str(int(q)) for q in v]
                f.write((" ".join(vals) + "\n").encode())
        else:
            rec = np.dtype([(name, cols[name].dtype.newbyteorder("<"), (3,) if name == "normal" else ()) for name in layout])
            arr = np.zeros(n, rec)
            for name in layout:
                arr[name] = cols[name]
            f.write(arr.tobytes())
    return str(path)


def same(got, xyz):
    want = xyz.reshape(H, W, 3)
    nan = np.isnan(want)
    return (got.dtype == np.float32 and got.shape == (H, W, 3) and got.flags["C_CONTIGUOUS"] and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


@pytest.mark.parametrize("data", ["ascii", "binary"])
@pytest.mark.parametrize("layout", [("x", "y", "z"), ("rgb", "x", "y", "z"), ("x", "y", "z", "rgb"), ("label", "x", "normal", "y", "rgb", "z")],
                         ids=["xyz", "rgb-first", "rgb-last", "interleaved"])
def test_reads_what_was_written(tmp_path, data, layout):
    xyz = points()
    assert np.isnan(xyz).all(1).any()
    path = write_pcd(tmp_path / "a.pcd", xyz, data, layout)
    assert same(read_pcd_xyz(path, H, W), xyz)                      # repr(float(float32)) round-trips: ascii is exact too


def test_header_variants(tmp_path):
    xyz = points(3)
    # unorganised header of the same count, no VIEWPOINT, upper-case DATA value
    path = write_pcd(tmp_path / "b.pcd", xyz, "binary", width=H * W, height=1, viewpoint=False)
    assert same(read_pcd_xyz(path, H, W), xyz)
    raw = open(path, "rb").read().replace(b"DATA binary", b"DATA BINARY")
    open(path, "wb").write(raw)
    assert same(read_pcd_xyz(path, H, W), xyz)


def test_refusals(tmp_path):
    xyz = points()
    ok = write_pcd(tmp_path / "ok.pcd", xyz, "binary")
    comp = str(tmp_path / "comp.pcd")
    open(comp, "wb").write(open(ok, "rb").read().replace(b"DATA binary", b"DATA binary_compressed"))
    with pytest.raises(ValueError, match=r"comp\.pcd.*binary_compressed"):
        read_pcd_xyz(comp, H, W)
    with pytest.raises(ValueError, match=r"ok\.pcd.*15 points"):       # the file is fine, the frame is another
        read_pcd_xyz(ok, H, W + 1)
    short = write_pcd(tmp_path / "short.pcd", xyz[:10], "ascii", width=W, height=2)
    with pytest.raises(ValueError, match=r"short\.pcd.*10 points"):
        read_pcd_xyz(short, H, W)
    lying = write_pcd(tmp_path / "lying.pcd", xyz[:10], "binary")      # header says 15, the data holds 10
    open(lying, "wb").write(open(lying, "rb").read().replace(b"POINTS 10", b"POINTS 15"))
    with pytest.raises(ValueError, match=r"lying\.pcd"):
        read_pcd_xyz(lying, H, W)
    noz = write_pcd(tmp_path / "noz.pcd", xyz, "ascii", layout=("x", "y", "rgb"))
    with pytest.raises(ValueError, match=r"noz\.pcd.*'z'"):
        read_pcd_xyz(noz, H, W)
    dbl = str(tmp_path / "dbl.pcd")
    open(dbl, "wb").write(open(ok, "rb").read().replace(b"SIZE 4 4 4", b"SIZE 8 4 4"))
    with pytest.raises(ValueError, match=r"dbl\.pcd.*'x'"):
        read_pcd_xyz(dbl, H, W)
    junk = str(tmp_path / "junk.pcd")
    open(junk, "wb").write(b"not a point cloud")
    with pytest.raises(ValueError, match=r"junk\.pcd"):
        read_pcd_xyz(junk, H, W)
