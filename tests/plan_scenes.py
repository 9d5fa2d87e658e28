"""Seeded worlds whose own size drives the bounce-level engine's launch plan
(csrc/rtx_plan.h) down each of its branches: tests/test_level_plans.py holds
the host's plan of every row of tests/golden/level_plans.json to the committed
one, tests/test_gpu_plans.py renders the rows.

make(n_sphere, n_light, seed): n_sphere spheres of mixed diffuse / mirror /
glass materials over the ground plane, one box, n_light lights (about a third
of them point lights) above and beside the field, so the ground has lit and
shadowed parts.  The spheres come from their own random stream, one after the
other: the world of n + 1 spheres is the world of n plus one sphere (the 512 /
513 pair around the host build's switch, rtx_scene_build.h small_scene).
hide_last moves that last sphere under the ground behind the camera, where no
camera ray, bounce or shadow ray to a light passes.  around spreads the
spheres over x in [-20, 20], behind the camera too: a field centred on the
origin is the shape whose 16-bit leaf records miss their error bound
(rtx_bvh_build.h quantize_leaves: half a step of 40 / 65535 against 1e-5 of
the scene's scale, about 26), so SceneDev::q_ok is 0 and a large hierarchy
takes SPH_BVH_MIX instead of SPH_BVH_QLDS.

multi_highlight(n_light, k): k of the lights on the camera's axis, one behind
the other with nothing in front, the others off the axis: the central rays fire
k highlights at once (world.rb:83-98, one leaf per fired light)."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_scenes  # noqa: E402

HEAD = "max_distance:           10000\nsoft_shadow_exponent:   2\n"
HIDDEN = [-40.0, 3.0, -30.0]       # under the ground (z = -1), behind the camera (at the origin, looking along +x)


def _light(name, pos, radius, color, rate, angle):
    return ("  - type: Spot\n    properties:\n"
            "      name:             %s\n      position:         %s\n      radius:           %s\n"
            "      color:            %s\n      high_light_rate:  %s\n      high_light_angle: %s\n"
            % (name, make_scenes.vec(pos), make_scenes.f(radius), make_scenes.vec(color), make_scenes.f(rate),
               make_scenes.f(angle)))


def _box(point):
    return ("  - type: Box\n    properties:\n      name: box\n      point: %s\n"
            "      front: [0.6, 0.8, 0.0]\n      up: [0.0, 0.0, 1.0]\n"
            "      width_front: 0.8\n      width_up: 1.1\n      width_left: 0.5\n"
            "      diffuse_rate: [0.5, 0.4, 0.3]\n      ambient: [0.02, 0.02, 0.02]\n"
            "      reflective_attenuation: [0.1, 0.1, 0.1]\n") % make_scenes.vec(point)


def world_text(n_sphere, n_light, seed, hide_last=False, around=False):
    rl = np.random.RandomState(100003 + seed)
    text = HEAD + ("lights:\n" if n_light else "")
    for k in range(n_light):
        # every third light a point light; low lights beside the field cast long shadows over the ground
        radius = 0.0 if k % 3 == 1 else rl.uniform(0.2, 0.9)
        pos = [rl.uniform(2, 18), rl.uniform(-9, 9), rl.uniform(2.5, 9)]
        text += _light("l%d" % k, pos, radius, rl.uniform(0.5, 0.95, 3), rl.uniform(0.3, 0.9), rl.uniform(0.5, 3.0))
    text += "world_objects:\n"
    rs = np.random.RandomState(seed)
    shrink = 1.0 if n_sphere <= 600 else (600.0 / n_sphere) ** (1.0 / 3.0)
    for i in range(n_sphere):
        c = [rs.uniform(3, 20), rs.uniform(-8, 8), rs.uniform(-1, 4)]
        if around:                 # a flat field on both sides of the camera (see the module's text)
            c = [rs.uniform(-20, 20), rs.uniform(-4, 4), rs.uniform(-1, 2)]
        r = rs.uniform(0.05, 0.4) * shrink
        mat = make_scenes.material(rs, int(rs.choice([0, 0, 1, 2])))
        if hide_last and i == n_sphere - 1:
            c = HIDDEN
        text += make_scenes.sphere("s%04d" % i, c, r, mat)
    return text + make_scenes.GROUND.format(extra="") + _box([7.0, 1.5, 0.2])


def camera_text(pt=1, depth=3, width=48, height=27):
    return ("position: [0.0, 0.0, 0.0]\nup: [0.0, 0.0, 1.0]\nfront: [1.0, 0.0, 0.0]\n"
            "retina_width: 0.016\nretina_height: 0.009\naperture_radius: 0.001\n"
            "image_distance: 0.01714573877962683\nfocal_distance: 0.017\n"
            "width: %d\nheight: %d\npre_sample_times: 2\nmax_sample_times: 3\nvariant_threshold: 0.001\n"
            "trace_depth: %d\nmonte_carlo_diffusion_times: %d\n" % (width, height, depth, pt))


def _write(out_dir, name, world, camera):
    w = os.path.join(str(out_dir), "%s_world.yml" % name)
    c = os.path.join(str(out_dir), "%s_camera.yml" % name)
    with open(w, "w") as f:
        f.write(world)
    with open(c, "w") as f:
        f.write(camera)
    return w, c


def make(n_sphere, n_light, seed, out_dir, hide_last=False, around=False, pt=1, depth=3):
    """(world.yml, camera.yml) written to out_dir."""
    name = "plan_%d_%d_%d%s%s" % (n_sphere, n_light, seed, "_hidden" if hide_last else "", "_around" if around else "")
    return _write(out_dir, name, world_text(n_sphere, n_light, seed, hide_last, around), camera_text(pt, depth))


HL_ANGLE = 6.0                     # degrees: the central 4 x 3 pixels' rays (at most 1.6 degrees off the axis
                                   # with the aperture's 0.001 / 0.017) fire every axis light


def multi_highlight_text(n_light, k):
    assert 1 <= k <= n_light
    rl = np.random.RandomState(7 * n_light + k)
    text = HEAD + "lights:\n"
    for j in range(n_light):
        if j < k:                  # on the axis, one behind the other
            pos, radius = [6.0 + 1.5 * j, 0.0, 0.0], (0.0 if j % 3 == 1 else 0.3)
        else:                      # off the axis by far more than the angle: at least 25 degrees
            a = rl.uniform(0, 2 * np.pi)
            pos, radius = [8.0, 8.0 * np.cos(a) + 0.0, 8.0 * abs(np.sin(a)) + 4.0], (0.0 if j % 3 == 1 else 0.5)
        # rates and colours below 1: the k leaves att * colour * rate / k of a ray sum to at most 0.9 a channel
        text += _light("l%d" % j, pos, radius, rl.uniform(0.5, 1.0, 3), rl.uniform(0.5, 0.9), HL_ANGLE)
    text += "world_objects:\n"
    rs = np.random.RandomState(n_light)
    for i in range(40):            # beside and below the axis, none within 1.2 of it
        c = [rs.uniform(4, 16), rs.choice([-1, 1]) * rs.uniform(2.0, 6.0), rs.uniform(-0.8, 1.5)]
        text += make_scenes.sphere("s%02d" % i, c, rs.uniform(0.2, 0.7), make_scenes.material(rs, int(rs.choice([0, 1, 2]))))
    return text + make_scenes.GROUND.format(extra="") + _box([9.0, -3.0, -0.4])


def make_multi_highlight(n_light, k, out_dir):
    return _write(out_dir, "hl_%d_%d" % (n_light, k), multi_highlight_text(n_light, k), camera_text())


# ---------------------------------------------------------------- the plan table
# tests/golden/level_plans.json: per row the generator's parameters, the scalars of SceneDev the
# plan depends on and the packed plan (rtx_plan.h pack_plan) that tools/scene_dump.cpp --plan
# printed for the row's world.  The rows are the smallest sphere counts of seed 11 that reach
# each plan (found by running the tool over 20 .. 4096 spheres); `python tests/plan_scenes.py`
# rewrites the file from ROWS.
SEED = 11
ROWS = (                           # name, n_sphere, n_light, around, pt, depth
    ("lin_20_l2", 20, 2, False, 1, 3),          # below bvh_min: the ordered linear walk
    ("ldsx_32_l4", 32, 4, False, 1, 3),         # light buffer and gates in LDS
    ("ldsx_64_l1", 64, 1, False, 3, 4),         # the same with path tracing children, one level more
    ("ldsx_48_l4", 48, 4, False, 1, 3),         # light buffer in LDS, gates from global memory
    ("ldsx_48_l16", 48, 16, False, 1, 3),       # ... and the light buffer ends at byte 163,840: no claim counter
    ("ldsx_32_l17", 32, 17, False, 1, 3),
    ("ldsx_32_l32", 32, 32, False, 1, 3),       # 8192 words hold no light buffer of 32 lights: none built
    ("ldsx_56_l4", 56, 4, False, 1, 3),         # a light buffer is built and does not fit
    ("ldsx_40_l0", 40, 0, False, 1, 3),
    ("lds_93_l2", 93, 2, False, 1, 3),          # the exact records no longer fit: SPH_BVH_LDS, full ring
    ("lds_512_l17", 512, 17, False, 1, 3),
    ("lds_513_l17", 513, 17, False, 1, 3),      # the host build's switch: global buffers, per-sphere raise lists
    ("lds_533_l2", 533, 2, False, 1, 3),        # the full ring ends at byte 163,840: no claim counter
    ("lds_536_l32", 536, 32, False, 1, 3),      # the compact ring
    ("qlds_1504_l2", 1504, 2, False, 1, 3),     # 16-bit leaf records, the raise check through the global buffers
    ("qlds_1504_l0", 1504, 0, False, 1, 3),     # ... and without buffers: the widened walk
    ("mix_1489_l2", 1489, 2, True, 1, 3),       # q_ok 0: the leaves from global memory
)
SCALARS = ("n_sphere", "n_light", "n_obj", "n_nodes", "n_slots", "bvh_stack", "q_ok", "lbuf_n", "lbuf_stride", "rbuf_n",
           "rgate_stride", "rbuf_sphere")


def unpack_plan(p):
    """The fields of a packed plan (rtx_plan.h pack_plan)."""
    return dict(mode=p & 15, ring=(p >> 4) & 15, lbuf=(p >> 8) & 1, rgate=(p >> 9) & 1, xr=(p >> 10) & 3,
                sched=(p >> 12) & 1, lds=p >> 16)


def row_world(row, out_dir, hide_last=False):
    return make(row["n_sphere"], row["n_light"], row["seed"], out_dir, hide_last=hide_last, around=row["around"],
                pt=row["pt"], depth=row["depth"])


def build_tool(out_dir):
    """tools/scene_dump.cpp compiled with g++ into out_dir."""
    import subprocess
    exe = os.path.join(str(out_dir), "scene_dump")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tools", "scene_dump.cpp"), "-lz", "-lpthread"], check=True, timeout=300)
    return exe


def host_plans(exe, worlds):
    """[(packed plan, {scalar: value})] of scene_dump --plan over the worlds; a refused world gives
    (None, "status <code> <message>")."""
    import subprocess
    p = subprocess.run([exe, "--plan"] + list(worlds), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout, p.stderr)
    out = []
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] != "plan":
            out.append((None, line))
            continue
        out.append((int(f[1]), {k: int(v) for k, v in zip(f[2::2], f[3::2])}))
    assert len(out) == len(worlds), p.stdout
    return out


def table(exe, out_dir):
    rows = [dict(name=n, n_sphere=ns, n_light=nl, seed=SEED, around=ar, pt=pt, depth=d) for n, ns, nl, ar, pt, d in ROWS]
    for row, (plan, scalars) in zip(rows, host_plans(exe, [row_world(r, out_dir)[0] for r in rows])):
        assert plan is not None, scalars
        row["scalars"] = {k: scalars[k] for k in SCALARS}
        row["plan"] = plan
    return rows


if __name__ == "__main__":
    import json
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        rows = table(build_tool(d), d)
    with open(os.path.join(ROOT, "tests", "golden", "level_plans.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    for r in rows:
        print(r["name"], r["plan"], unpack_plan(r["plan"]))
