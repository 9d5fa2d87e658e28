"""Worlds whose ray trees are deep and narrow, for tests/test_deep_trees.py (the
conditions, on the oracles alone) and tests/test_gpu_deep_trees.py (the renders).

A tree that is to fill a walk's stack has to leave something pending at every
level and still be small enough to render at trace_depth 64: a few thousand
rays a sample, not 3^64.

row (monte_carlo_diffusion_times 0): N glass spheres on the view axis, centres
(3 + i, 0, 0), radius 0.4.  The refractions form the chain (attenuation 0.97 a
hit, two hits a sphere); every hit leaves its reflection pending (pushed first,
ray_tracer.rb:104-118, so it waits while the refraction's subtree runs) with
attenuation 0.004: alive, and its own reflection (0.004^2) under the 1e-4
cutoff.  One point light far to the side lights the outer hits.  The pending
stack of the lanes engine peaks at trace_depth - 1 = required_stack's need - 1.

shell (monte_carlo_diffusion_times > 0): the camera inside one large sphere.
Every hit is an :out hit whose shadow ray the sphere itself covers, so every hit
is unlit and makes its path-tracing children (world_object.rb:76-90), pushed
after the reflection and the refraction: while the last of them runs, 1 + pt
siblings are pending a level.  refractive_rate 0.9 < 1 leaves no total internal
reflection (sin_r = sin_i * 0.9), so both are there at every hit; the refracted
ray leaves the sphere and meets nothing.  The only leaves are highlights: a
light outside the sphere fires on every ray within high_light_angle of it
(world.rb:83-98 tests no occlusion), which also ends that ray's subtree.
diffuse_rate = rate * pt gives every path-tracing child the attenuation `rate`.
The trees of pt 14 and 15 are thinned by max_distance (SHELL below).
"""
import os
import sys

from conftest import ROOT
from plan_scenes import HEAD, _light, _write

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_scenes  # noqa: E402

N_ROW = 40
SEED = 5

# (trace_depth, monte_carlo_diffusion_times): the pt 0 cases around every switch of the tree reduction's
# walk stack (nlev 5 | 6, 8 | 9, 16 | 17) and of the lanes engine's stack buckets (need 8 | 9, 16 | 17,
# 32 | 33, 64), the ray record's 80 | 96 bytes (3^21 > 2^32; 4^16 = 2^32), the engine limit at pt 14 | 15.
# (10, 0), (18, 0), (34, 0) and (18, 1) sit one past the edges: a stack of SD or `bucket` entries holds
# the nlev - 1 = need - 1 entries that (9, 0), (17, 0), (33, 0) and (17, 1) can reach at most, so those
# run with a smaller stack than the code gives them and still fit; these do not.
CASES = ((5, 0), (6, 0), (8, 0), (9, 0), (10, 0), (16, 0), (17, 0), (18, 0), (20, 0), (21, 0), (32, 0), (33, 0),
         (34, 0), (64, 0), (16, 1), (17, 1), (18, 1), (32, 1), (5, 14), (4, 15))


def case_name(depth, pt):
    return "d%d_pt%d" % (depth, pt)


def need(depth, pt):
    """required_stack's entry count (rtx_capi.cpp): 1 + (depth - 1) * (1 + pt)."""
    return 1 + max(depth - 1, 0) * (1 + pt)


def bucket(n):
    """stack_bucket (rtx_kernels.hip)."""
    return next((b for b in (8, 16, 32, 64) if n <= b), -1)


def _sphere(name, centre, radius, rate, diffuse, ambient, refl, refr):
    return ("  - type: Sphere\n    properties:\n      name: %s\n      center: %s\n      radius: %s\n"
            "      refractive_rate: %s\n      diffuse_rate: %s\n      ambient: %s\n"
            "      reflective_attenuation: %s\n      refractive_attenuation: %s\n"
            % (name, make_scenes.vec(centre), make_scenes.f(radius), make_scenes.f(rate), make_scenes.vec([diffuse] * 3),
               make_scenes.vec([ambient] * 3), make_scenes.vec([refl] * 3), make_scenes.vec([refr] * 3)))


def row_world_text(n=N_ROW):
    text = HEAD + "lights:\n" + _light("side", [22.0, -300.0, 40.0], 0.0, [0.9, 0.9, 0.9], 0.5, 3.0) + "world_objects:\n"
    for i in range(n):
        text += _sphere("g%02d" % i, [3.0 + i, 0.0, 0.0], 0.4, 1.05, 0.02, 0.01, 0.004, 0.97)
    return text


# shell worlds per pt: the path-tracing child's attenuation, the highlight's half angle (degrees) and
# colour x rate, the world's max_distance.  pt 1: a narrow cone, so a chain of 31 path-tracing rays
# survives in some sample and one that ends in the cone adds 0.9^31 * 0.72 = 0.027 at the last level.
# pt 14 / 15: 16^4 rays a sample times 48 would not fit the level buffers, and ending them in a wide cone
# would overflow the deferred highlight checks' list (samples re-rendered: rtx_level_stats' redo).  A
# max_distance of 58.8 = 100 sin(36 deg) instead ends every ray that leaves the shell's surface more than
# 36 degrees above the tangent, three in five (theta is uniform, world_object.rb:84): World#intersect takes
# no hit at or beyond max_distance (world.rb:38-53), the shadow rays know no such limit.
SHELL = {1: (0.9, 15.0, 0.72, 10000.0), 14: (0.3, 15.0, 0.1, 58.8), 15: (0.3, 15.0, 0.1, 58.8)}


def shell_world_text(pt):
    rate, angle, c, max_distance = SHELL[pt]
    text = ("max_distance:           %s\nsoft_shadow_exponent:   2\n" % make_scenes.f(max_distance) + "lights:\n" +
            _light("zenith", [30.0, 40.0, 200.0], 0.0, [c / 0.8] * 3, 0.8, angle) + "world_objects:\n")
    return text + _sphere("shell", [0.0, 0.0, 0.0], 50.0, 0.9, rate * pt, 0.01, 0.004, 0.05)


def world_text(pt):
    return row_world_text() if pt == 0 else shell_world_text(pt)


def camera_text(depth, pt, width=8, height=6):
    return ("position: [0.0, 0.0, 0.0]\nup: [0.0, 0.0, 1.0]\nfront: [1.0, 0.0, 0.0]\n"
            "retina_width: 0.0016\nretina_height: 0.0012\naperture_radius: 0.0001\n"
            "image_distance: 0.01714573877962683\nfocal_distance: 0.017\n"
            "width: %d\nheight: %d\npre_sample_times: 1\nmax_sample_times: 1\nvariant_threshold: 1000.0\n"
            "trace_depth: %d\nmonte_carlo_diffusion_times: %d\n" % (width, height, depth, pt))


def make(depth, pt, out_dir, width=8, height=6):
    """(world.yml, camera.yml) of the case written to out_dir."""
    return _write(out_dir, "deep_%s_%dx%d" % (case_name(depth, pt), width, height), world_text(pt),
                  camera_text(depth, pt, width, height))


def load(depth, pt, out_dir, width=8, height=6):
    """The case's flat descriptors (raytracing_rb_amd.config)."""
    from raytracing_rb_amd import config
    return config.load_scene(*make(depth, pt, out_dir, width, height))


def fixture():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "deep_trees.json")) as f:
        return {r["name"]: r for r in json.load(f)}


WIDE = ((64, 0), (17, 1))          # also recorded at 16 x 10: two 8 x 8 tiles a row (lv_streams, lv_fin_grid)


def rows():
    """(name, depth, pt, width, height) of every fixture row."""
    out = [(case_name(d, pt), d, pt, 8, 6) for d, pt in CASES]
    return out + [(case_name(d, pt) + "_16x10", d, pt, 16, 10) for d, pt in WIDE]


def measure(depth, pt, out_dir, width=8, height=6):
    """A fixture row's recorded values, by the C oracle: the frame's peak of pending siblings and the samples
    that reach it (rt_map_tree.max_pending's discipline, Oracle.tree_stats), the rays per tree level, their sum."""
    from oracle.c_oracle import Oracle
    o = Oracle(*load(depth, pt, out_dir, width, height))
    pend, levels, status, rc = o.tree_stats(seed=SEED)
    assert rc == 0 and not status.any(), (depth, pt, o.last_error())
    return {"max_pending": int(pend.max()), "samples_at_max": int((pend == pend.max()).sum()),
            "rays_per_level": [int(v) for v in levels], "rays": int(levels.sum())}
