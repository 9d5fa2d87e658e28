"""The worlds of tests/test_scene_build.py: the committed scenes, fuzz and posed
seeds (fuzz_scenes.py) and hand-made edges of rtx_scene_upload's host build.
tests/golden/scene_build.json records, per world, what the parent of the host
scene build (7697613) sent to the device for it."""
import os
import sys

import numpy as np

import fuzz_scenes
from conftest import ROOT, SCENES

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_scenes  # noqa: E402

HEAD = "max_distance:           10000\nsoft_shadow_exponent:   %s\n"
MAT = ([0.5] * 3, [0.05] * 3, [0.3] * 3, [0.1] * 3)


def _lights(*ls):
    out = "lights:\n"
    for k, (pos, radius) in enumerate(ls):
        out += make_scenes.light(pos, radius).split("\n", 1)[1].replace("Main", "l%d" % k)
    return out


def _box(point):
    return ("  - type: Box\n    properties:\n      name: box\n      point: %s\n"
            "      front: [0.6, 0.8, 0.0]\n      up: [0.0, 0.0, 2.0]\n"
            "      width_front: 0.8\n      width_up: 1.1\n      width_left: 0.5\n"
            "      diffuse_rate: [0.5, 0.4, 0.3]\n      ambient: [0.02, 0.02, 0.02]\n"
            "      reflective_attenuation: [0.1, 0.1, 0.1]\n") % make_scenes.vec(point)


def _edges():
    ground = make_scenes.GROUND.format(extra="")
    ball = make_scenes.sphere("ball", [5.0, 0.5, 0.25], 0.75, MAT)
    yield "no_spheres", (HEAD % 2 + _lights(([4.0, -3.0, 5.0], 0.5)) + "world_objects:\n" + ground
                         + _box([6.0, 1.0, 0.0]))
    yield "no_lights", HEAD % 2 + "world_objects:\n" + ball + ground
    yield "one_sphere", HEAD % 3 + _lights(([2.0, -3.0, 4.0], 0.6)) + "world_objects:\n" + ball
    # a light inside a sphere: that sphere's leaf in every cell of both buffers
    yield "light_in_sphere", (HEAD % 2 + _lights(([5.0, 0.25, 0.5], 0.3), ([1.0, 4.0, 6.0], 0.0)) + "world_objects:\n"
                              + ball + make_scenes.sphere("other", [7.0, -2.0, 0.0], 0.5, MAT) + ground)
    # above 512 spheres: the buffers read from global memory, per-sphere raise lists, two area lights
    rs = np.random.RandomState(600)
    many = "".join(make_scenes.sphere("s%03d" % i, [rs.uniform(3, 20), rs.uniform(-8, 8), rs.uniform(-1, 4)],
                                      rs.uniform(0.05, 0.4), MAT) for i in range(600))
    yield "many_two_lights", (HEAD % 2 + _lights(([6.0, -4.0, 9.0], 0.8), ([15.0, 5.0, 7.0], 0.4))
                              + "world_objects:\n" + many + ground + _box([10.0, 0.0, 5.0]))


def worlds(out_dir, with_c4=False):
    """{name: path of its world.yml}, generated files in out_dir."""
    out = {n: os.path.join(SCENES, "%s_world.yml" % n) for n in ("c0", "c1", "c2", "mix")}
    if with_c4:
        out["c4"] = make_scenes.ensure_c4()
    for seed in range(6):
        out["fuzz%d" % seed] = fuzz_scenes.make(seed, out_dir)[0]
    for seed in range(4):
        out["posed%d" % seed] = fuzz_scenes.make_posed(seed, out_dir)[0]
    for name, text in _edges():
        out[name] = os.path.join(str(out_dir), "%s_world.yml" % name)
        with open(out[name], "w") as f:
            f.write(text)
    return out


def parse_dump(text):
    """scene_dump's output: {"arrays": {name: [bytes, fnv1a]}, "scalars": {name: text}}."""
    d = {"arrays": {}, "scalars": {}}
    for line in text.splitlines():
        f = line.split()
        if f[0] == "array":
            d["arrays"][f[1]] = [int(f[2]), f[3]]
        else:
            assert f[0] == "scalar", line
            d["scalars"][f[1]] = f[2]
    return d
