"""The host scene build (csrc/rtx_scene_build.h) sends the device what
rtx_scene_upload sent before it was split out.

tests/golden/scene_build.json holds, per world of scene_build_cases.py, the
byte count and 64-bit FNV-1a hash of every array and every scalar of SceneDev
(floats as hex) that the upload of commit 7697613 copied, recorded from that
commit's rtx_capi.cpp (hipcc host build) with host stand-ins for its HIP
calls.  tools/scene_dump.cpp prints the same table from build_host_scene under
plain g++, so the test also holds the g++ build of the header to the library's
hipcc build.  The table's c4 entry (2 s and 79 MB to build) is compared by hand;
tests/test_lbuf.py runs the c4 build at full size."""
import json
import os
import shutil
import subprocess

import pytest

import scene_build_cases
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("scene_build")
    exe = str(d / "scene_dump")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tools", "scene_dump.cpp"), "-lz", "-lpthread"], check=True, timeout=300)
    out = {}
    for name, world in scene_build_cases.worlds(d).items():
        p = subprocess.run([exe, world], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (name, p.stdout, p.stderr)
        out[name] = scene_build_cases.parse_dump(p.stdout)
    return out


with open(os.path.join(GOLDEN, "scene_build.json")) as _f:
    TABLE = json.load(_f)


def test_the_table_covers_the_branches():
    s = {n: t["scalars"] for n, t in TABLE.items()}
    assert s["no_spheres"]["n_sphere"] == "0" and s["no_lights"]["n_light"] == "0" and s["one_sphere"]["n_sphere"] == "1"
    assert s["no_spheres"]["lbuf_n"] == s["no_lights"]["lbuf_n"] == "0"
    many = s["many_two_lights"]
    assert int(many["n_sphere"]) > 512 and many["n_light"] == "2" and many["rbuf_sphere"] == "1" and int(many["rbuf_n"]) > 0
    assert any(int(t["n_box"]) > 0 for t in s.values()) and any(TABLE[n]["arrays"]["texels"][0] > 0 for n in TABLE)


@pytest.mark.parametrize("name", [n for n in TABLE if n != "c4"])
def test_host_scene_equals_the_parent_upload(dumps, name):
    assert set(dumps) == set(TABLE) - {"c4"}
    want, got = TABLE[name], dumps[name]
    assert got["arrays"] == want["arrays"]
    assert got["scalars"] == want["scalars"]
