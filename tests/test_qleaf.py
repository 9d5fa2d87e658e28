"""SPH_BVH_QLDS's 16-bit leaf records hold every true sphere.

The host half of rtx_scene_upload (sphere packing, hierarchy build and
quantize_leaves: csrc/rtx_scene_build.h) runs in tools/qleaf_check.cpp,
compiled here with g++ (host code only, no GPU call).  For every occupied slot the float32 ball the device
decodes must contain the true binary64 ball, checked in exact rational
arithmetic: r' >= R and (r' - R)^2 >= |c - c'|^2.  When the scene passes the
host's check (q_ok), the largest center error is at most half the pre-test's
margin m S (S >= the scene's sphere scale).  The GPU tests (test_gpu_bvh.py,
test_gpu_levels.py) check the frames: the same bits with sphere_src 4.
"""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, SCENES

CULL_M = Fraction(float(np.float32(2e-5)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("qleaf") / "qleaf_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-o", exe, os.path.join(ROOT, "tools", "qleaf_check.cpp"),
                    "-lpthread"], check=True, timeout=600)
    return exe


def _run(tool, spheres, sah=0):
    text = "".join("%r %r %r %r\n" % tuple(float(v) for v in s) for s in spheres)
    out = subprocess.run([tool, str(sah)], input=text, capture_output=True, text=True, check=True, timeout=120).stdout
    lines = out.strip().splitlines()
    tail = lines[-1].split()
    assert tail[0] == "ok"
    rows = [[Fraction(float.fromhex(v)) for v in l.split()] for l in lines[:-1]]
    return rows, tail[1] == "1", Fraction(float.fromhex(tail[2])), Fraction(float.fromhex(tail[3]))


def _check(tool, spheres, sah=0, want_ok=None):
    rows, ok, max_err, scale = _run(tool, spheres, sah)
    assert len(rows) == len(spheres)
    for cx, cy, cz, R, dx, dy, dz, dr in rows:
        e2 = (cx - dx) ** 2 + (cy - dy) ** 2 + (cz - dz) ** 2
        assert dr >= R and (dr - R) ** 2 >= e2, (cx, cy, cz, R, dx, dy, dz, dr)
    if ok:
        assert max_err <= CULL_M * scale / 2
    if want_ok is not None:
        assert ok == want_ok
    return ok


def _c4_spheres():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_scenes
    from raytracing_rb_amd import config
    sd, _ = config.load_scene(make_scenes.ensure_c4(), os.path.join(SCENES, "c4_camera.yml"))
    d = sd.desc
    return [tuple(d.objects[i].center) + (d.objects[i].radius,) for i in range(d.n_objects) if d.objects[i].type == 0]


def test_c4_quantized_leaves_hold_the_spheres(tool):
    assert _check(tool, _c4_spheres(), want_ok=True)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("sah", [0, 1])
def test_random_scenes(tool, seed, sah):
    rs = np.random.RandomState(seed)
    n = rs.randint(5, 400)
    c = rs.uniform(-50, 50, (n, 3)) * rs.uniform(0.01, 1, (1, 3))
    r = rs.uniform(0.01, 2.0, n)
    _check(tool, [tuple(c[k]) + (r[k],) for k in range(n)], sah)


def test_edge_scenes(tool):
    _check(tool, [(3.0, -1.0, 0.5, 0.4)], want_ok=True)                       # one sphere: a zero extent
    _check(tool, [(1.0, 2.0, 3.0, 0.5)] * 9, want_ok=True)                    # identical spheres
    _check(tool, [(0.0, 0.0, 0.0, 1e-3), (1e-7, 0.0, 0.0, 1e-3), (5.0, 5.0, 5.0, 2.0)])
    # centers a million units apart: the 16-bit grid is too coarse for the
    # pre-test's margin, the host refuses the mode (SPH_BVH_MIX instead)
    _check(tool, [(-1e6, 0.0, 0.0, 0.5), (1e6, 3.0, 0.0, 0.5), (0.0, 1e6, 7.0, 1.0), (1.0, 1.0, 1.0, 1.0)],
           want_ok=False)
