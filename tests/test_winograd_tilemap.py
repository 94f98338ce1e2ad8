"""The tile map of the dilated Winograd layers (quber_amd/csrc/winograd_xf.h: Axis) on the host: tests/host/wino_tilemap_main.hip is a
stand-alone program on the host instance of the functions the transform kernels call.  For every H, W in 1..48, d in 1..20 and
m in {2, 4, 6} it checks that every pixel of an axis is the output slot of exactly one tile, that the slots before and after an
output slot are the pixel's neighbours in its phase (or zero at the phase's ends), that the tile count is the smaller of the per-phase
and the packed one, and the counts of the 30x40 and 45x80 maps.  No GPU is needed: only the host half is compiled."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("hipcc not found: the library itself cannot be built without it")


def test_winograd_tile_map_host(tmp_path):
    exe = str(tmp_path / "wino_tilemap")
    src = os.path.join(ROOT, "tests", "host", "wino_tilemap_main.hip")
    subprocess.run([_hipcc(), "-std=c++17", "-O1", "--offload-arch=gfx950", "--cuda-host-only", src, "-o", exe], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "tile map ok" in r.stdout
