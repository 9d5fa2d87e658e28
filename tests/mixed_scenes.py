"""Worlds of many planes and boxes in mixed YAML order (test_mixed_scenes.py on
the CPU, test_gpu_mixed.py on the GPU): the code that walks planes and boxes
and merges them with the sphere results (csrc/rtx_device.h walk_planes_boxes,
lex_better, push_cover, query()'s groups of four) under closed views, where
every ray has a far bound.

make(seed, n_sphere, n_box, out_dir): a seeded closed room.  Six wall planes
around the camera and the field (the floor textured, the back wall on some
seeds), one tilted refractive plane through the field (a glass pane), n_box
boxes whose front and up come from a random rotation with non-unit lengths
(some refractive), n_sphere spheres in diffuse / mirror / glass materials.
Every sunk_every-th sphere (every fifth by default; every second in the rooms
of 40 and 100 spheres, the share their near-tie condition needs at 48 x 27) is
sunk into a wall or a box face that looks at the camera, its centre within 0.1
of the surface: five in six are shallow caps (the centre behind the surface,
0.03 to 0.04 of the sphere in front of it, or 0.002 to 0.006: the hit lies
within a hair of the far bound the surface sets), the sixth a large ball about
half sunk.  Two or three lights inside the room, the first a point light.  All
objects are shuffled into one YAML order.  The worlds are small (S): at 48 x 27
a cap 0.04 high must still fill pixels.

The hand-made worlds: sphere_runs, twins, no_spheres, inside_box, flush and
cover_stacks(order, fillers) (see each function).

first_hits() and CoverCount are the oracle's (oracle/rt_ref.py) own
account of a world: what wins each lens ray and by how much, and how many
covers of which kinds a shadow query meets.  `python tests/mixed_scenes.py`
rewrites tests/golden/mixed_scenes.json from them."""
import functools
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TEXTURES = os.path.join(ROOT, "scenes", "textures")
for _p in (ROOT, HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_scenes  # noqa: E402
from fuzz_scenes import _rotation, _v  # noqa: E402

COVER_K = 4                        # csrc/rtx_scene.h
NEAR = 0.05                        # a runner-up this close to the winner: a near-tie
S = 0.3                            # the worlds' scale: the room is 4.8 x 3.6 x 1.95, so that a cap 0.04 high fills pixels
X, Y, Z = (-2.0 * S, 14.0 * S), (-6.0 * S, 6.0 * S), (-1.5 * S, 5.0 * S)          # the room
#           name       point              front (inward)     up
WALLS = (("floor", (0.0, 0.0, Z[0]), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)),
         ("ceiling", (0.0, 0.0, Z[1]), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)),
         ("back", (X[1], 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0)),
         ("behind", (X[0], 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)),
         ("left", (0.0, Y[1], 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0)),
         ("right", (0.0, Y[0], 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)))
# seed, spheres, boxes, every n-th sphere sunk, trace_depth, monte_carlo_diffusion_times: sphere counts on both
# sides of bvh_min = 32; the sunk share is what test_mixed_scenes.py's near-tie condition needs
ROOMS = ((1, 3, 12, 5, 4, 1), (7, 40, 20, 2, 3, 2), (3, 100, 30, 2, 3, 1))


def _obj(kind, name, props):
    out = ["  - type: %s" % kind, "    properties:", "      name: %s" % name]
    for k, v in props:
        out.append("      %s: %s" % (k, v if isinstance(v, str) else (_v(v) if np.ndim(v) else repr(float(v)))))
    return "\n".join(out) + "\n"


def _mat(mat, glass_rate=None):
    d, a, rl, rr = mat
    out = [("diffuse_rate", d), ("ambient", a), ("reflective_attenuation", rl)]
    if glass_rate is not None:
        out += [("refractive_rate", glass_rate), ("refractive_attenuation", rr)]
    return out


def _texture(name, uu, vu, hs, vs):
    return [("u_unit", uu), ("v_unit", vu), ("texture_file_path", os.path.join(TEXTURES, name)),
            ("texture_horizontal_scale", hs), ("texture_vertical_scale", vs)]


def _plane(name, point, front, up, mat, glass_rate=None, extra=()):
    return _obj("Plane", name, [("point", point), ("front", front), ("up", up)] + _mat(mat, glass_rate) + list(extra))


def _box(name, point, front, up, widths, mat, glass_rate=None):
    return _obj("Box", name, [("point", point), ("front", front), ("up", up), ("width_front", widths[0]),
                              ("width_up", widths[1]), ("width_left", widths[2])] + _mat(mat, glass_rate))


def _sphere(name, c, r, mat, rate=1.5):
    d, a, rl, rr = mat
    return _obj("Sphere", name, [("center", c), ("radius", r), ("refractive_rate", rate), ("diffuse_rate", d),
                                 ("ambient", a), ("reflective_attenuation", rl), ("refractive_attenuation", rr)])


def _light(name, pos, radius, color, rate, angle):
    return ("  - type: Spot\n    properties:\n      name: %s\n      position: %s\n      radius: %r\n"
            "      color: %s\n      high_light_rate: %r\n      high_light_angle: %r\n"
            % (name, _v(pos), float(radius), _v(color), float(rate), float(angle)))


def _wall_mat(rs):
    """Walls: diffuse with a little reflection; d + a + refl <= 0.98 per channel (rt_reduce never raises)."""
    return rs.uniform(0.3, 0.65, 3), [0.03] * 3, rs.uniform(0.05, 0.25, 3), [0.0] * 3


def walls(rs, textured=()):
    """The six wall planes; `textured` maps a wall's name to its texture's lines."""
    return [_plane(n, p, f, u, _wall_mat(rs), extra=dict(textured).get(n, ())) for n, p, f, u in WALLS]


def box_faces(point, front, up, widths):
    """(centre, unit normal, half extents along (a, b), a, b) of the six faces, in box.rb's order."""
    point, front, up = (np.array(t, float) for t in (point, front, up))
    left = np.cross(front, up)
    left /= np.linalg.norm(left)
    wf, wu, wl = widths
    out = []
    for axis, w, (a, wa), (b, wb) in ((up, wu, (front, wf), (left, wl)), (front, wf, (left, wl), (up, wu)),
                                      (left, wl, (front, wf), (up, wu))):
        for s in (1.0, -1.0):
            out.append((point + s * axis * w * 0.5, s * axis / np.linalg.norm(axis), (a * wa * 0.5, b * wb * 0.5)))
    return out


def camera_text(pt=1, depth=3, width=48, height=27, position=(0.0, 0.0, 0.0), front=(1.0, 0.0, 0.0),
                retina=(0.016, 0.009), pre=2, mx=3):
    return ("position: %s\nup: [0.0, 0.0, 1.0]\nfront: %s\n"
            "retina_width: %r\nretina_height: %r\naperture_radius: 0.001\n"
            "image_distance: 0.01714573877962683\nfocal_distance: 0.017\n"
            "width: %d\nheight: %d\npre_sample_times: %d\nmax_sample_times: %d\nvariant_threshold: 0.001\n"
            "trace_depth: %d\nmonte_carlo_diffusion_times: %d\n"
            % (_v(position), _v(front), retina[0], retina[1], width, height, pre, mx, depth, pt))


def _write(out_dir, name, world, camera):
    w = os.path.join(str(out_dir), "%s_world.yml" % name)
    c = os.path.join(str(out_dir), "%s_camera.yml" % name)
    with open(w, "w") as f:
        f.write(world)
    with open(c, "w") as f:
        f.write(camera)
    return w, c


HEAD = "max_distance: 10000\nsoft_shadow_exponent: 2\n"


def _room_lights(rs):
    text = "lights:\n"
    n = int(rs.randint(2, 4))
    for k in range(n):
        if k == 0:                 # a point light on the camera's side of the pane
            pos, radius = S * np.array([rs.uniform(2, 5), rs.uniform(-3, 3), rs.uniform(2.5, 4.5)]), 0.0
        elif k == 1:               # an area light behind it
            pos, radius = S * np.array([rs.uniform(10.5, 13), rs.uniform(-4, 4), rs.uniform(2, 4.5)]), S * rs.uniform(0.3, 0.9)
        else:
            pos, radius = S * np.array([rs.uniform(3, 12), rs.uniform(-5, 5), rs.uniform(3, 4.7)]), S * rs.uniform(0.3, 0.9)
        text += _light("l%d" % k, pos, radius, rs.uniform(0.5, 0.95, 3), rs.uniform(0.3, 0.9), rs.uniform(0.5, 3.0))
    return text


def _sunk_site(rs, boxes):
    """A point of a wall in view or of a box face, and the unit normal towards the room / out of the box."""
    if boxes and rs.rand() < 0.5:                  # a face that looks at the camera (at the origin)
        faces = [f for f in box_faces(*boxes[rs.randint(len(boxes))]) if f[0].dot(f[1]) < 0]
        c, n, (a, b) = faces[rs.randint(len(faces))]
        return c + rs.uniform(-0.6, 0.6) * a + rs.uniform(-0.6, 0.6) * b, n
    k = int(rs.choice([2, 2, 4, 5]))          # (not the floor: seen at a grazing angle)
    n = np.array(WALLS[k][2])
    p = S * np.array([rs.uniform(6.0, 12.5), rs.uniform(-4.5, 4.5), rs.uniform(-1.0, 3.0)])
    p[np.argmax(np.abs(n))] = np.array(WALLS[k][1])[np.argmax(np.abs(n))]
    return p, n


def room_text(seed, n_sphere, n_box, sunk_every=5):
    rs = np.random.RandomState(65537 * seed + n_sphere)
    text = HEAD + _room_lights(rs)
    tex = {"floor": _texture("checker.png", rs.uniform(0.5, 2.0), rs.uniform(0.5, 2.0), rs.uniform(0.01, 0.05),
                             rs.uniform(0.01, 0.05))}
    if rs.rand() < 0.5:
        tex["back"] = _texture("rails_synth.png", 1.0, 1.0, rs.uniform(0.01, 0.03), rs.uniform(0.01, 0.03))
    objs = walls(rs, tex)
    pane_front = np.array([-1.0, rs.uniform(-0.4, 0.4), rs.uniform(-0.3, 0.3)]) * rs.uniform(0.5, 2.0)
    objs.append(_plane("pane", [S * rs.uniform(8, 10), 0.0, 0.0], pane_front, [0.0, 0.3, 1.0],
                       (rs.uniform(0.02, 0.08, 3), [0.01] * 3, [0.1] * 3, rs.uniform(0.5, 0.8, 3)),
                       glass_rate=rs.uniform(1.2, 1.6)))
    boxes = []
    for k in range(n_box):
        Q = _rotation(rs)
        geo = (S * np.array([rs.uniform(4, 13), rs.uniform(-5, 5), rs.uniform(-1.2, 4.0)]), Q[:, 0] * rs.uniform(0.5, 1.6),
               Q[:, 1] * rs.uniform(0.5, 1.6), S * rs.uniform(0.3, 1.4, 3))
        kind = int(rs.choice([0, 0, 1, 2]))
        boxes.append(geo)
        objs.append(_box("b%02d" % k, geo[0], geo[1], geo[2], geo[3], make_scenes.material(rs, kind),
                         glass_rate=rs.uniform(1.2, 1.7) if kind == 2 else None))
    shrink = 1.0 if n_sphere <= 40 else (40.0 / n_sphere) ** (1.0 / 3.0)
    for k in range(n_sphere):
        mat = make_scenes.material(rs, int(rs.choice([0, 0, 1, 2])))
        if k % sunk_every == sunk_every - 1:
            p, n = _sunk_site(rs, boxes)
            if (k // sunk_every) % 6 == 5:         # a large ball about half sunk
                off, r = rs.uniform(-0.1, 0.1), S * rs.uniform(0.3, 0.7)
            else:                                  # a shallow cap: the centre behind the surface, a hair
                off = -rs.uniform(0.09, 0.1)       # (every sixth: 0.002 to 0.006) or 0.03 to 0.04 of it in front
                r = -off + (rs.uniform(0.002, 0.006) if (k // sunk_every) % 6 == 2 else rs.uniform(0.03, 0.04))
            c = p + n * off
        else:
            c, r = S * np.array([rs.uniform(3.5, 13), rs.uniform(-5, 5), rs.uniform(-1.2, 4.0)]), S * rs.uniform(0.2, 0.8) * shrink
        objs.append(_sphere("s%03d" % k, c, r, mat, rate=rs.uniform(1.2, 1.7)))
    order = rs.permutation(len(objs))
    return text + "world_objects:\n" + "".join(objs[i] for i in order)


def make(seed, n_sphere, n_box, out_dir, sunk_every=5, depth=3, pt=1, width=48, height=27):
    """(world.yml, camera.yml) of a seeded closed room, written to out_dir."""
    return _write(out_dir, "room_%d_%d_%d" % (seed, n_sphere, n_box), room_text(seed, n_sphere, n_box, sunk_every),
                  camera_text(pt, depth, width, height))


def make_room(k, out_dir, width=48, height=27):
    seed, ns, nb, every, depth, pt = ROOMS[k]
    return make(seed, ns, nb, out_dir, every, depth, pt, width, height)


# ---------------------------------------------------------------- the hand-made worlds
def _spheres(rs, names, lo=(3.5, -4.5, -1.0), hi=(11.0, 4.5, 3.5)):
    return [_sphere(n, S * rs.uniform(lo, hi), S * rs.uniform(0.25, 0.7), make_scenes.material(rs, int(rs.choice([0, 0, 1, 2]))))
            for n in names]


def _plain_box(rs, name, kind=0, glass=False):
    Q = _rotation(rs)
    return _box(name, S * np.array([rs.uniform(4, 12), rs.uniform(-4.5, 4.5), rs.uniform(-1.0, 3.5)]), Q[:, 0] * rs.uniform(0.6, 1.5),
                Q[:, 1] * rs.uniform(0.6, 1.5), S * rs.uniform(0.5, 1.5, 3), make_scenes.material(rs, 2 if glass else kind),
                glass_rate=1.5 if glass else None)


TWO_LIGHTS = ("lights:\n" + _light("point", [3.0 * S, -2.0 * S, 4.0 * S], 0.0, [0.9, 0.9, 0.8], 0.8, 2.0)
              + _light("area", [9.0 * S, 3.0 * S, 4.2 * S], 0.7 * S, [0.8, 0.9, 0.9], 0.6, 1.5))
SPHERE_RUNS = (1, 2, 3, 5, 7, 1, 4)


def sphere_runs(out_dir, width=48, height=27):
    """Sphere runs of 1, 2, 3, 5, 7, 1 and 4 (23 spheres: the default walk is the ordered linear one),
    separated by single walls and boxes: records at rec0 = 0, 1, 3, 6, 11, 18, 19 in the padded table."""
    rs = np.random.RandomState(41)
    w = walls(rs, {"floor": _texture("checker.png", 1.0, 1.0, 0.02, 0.02)})
    sep = [w[0], _plain_box(rs, "b0"), w[1], _plain_box(rs, "b1", glass=True), w[2], w[3], _plain_box(rs, "b2", 1)]
    text, k = HEAD + TWO_LIGHTS + "world_objects:\n", 0
    for run, n in enumerate(SPHERE_RUNS):
        text += sep[run] + "".join(_spheres(rs, ["s%02d" % (k + j) for j in range(n)]))
        k += n
    text += w[4] + _plain_box(rs, "b3") + w[5]
    return _write(out_dir, "sphere_runs", text, camera_text(1, 3, width, height))


def twins(out_dir, width=48, height=27):
    """Exact ties between equal kinds and near-ties between kinds: a pane and a box each written twice
    with different materials (the lower index wins), a box behind the left wall with one face in the
    left wall's plane, a box standing on the floor (its bottom face in the floor's plane), a sphere tangent
    to the right wall and one tangent to the floor."""
    rs = np.random.RandomState(43)
    w = walls(rs)
    red, green = ([0.7, 0.1, 0.1], [0.02] * 3, [0.1] * 3, [0.0] * 3), ([0.1, 0.7, 0.1], [0.02] * 3, [0.2] * 3, [0.0] * 3)
    pane = ([3.3, 0.0, 0.0], [-1.0, 0.2, 0.1], [0.0, 0.0, 1.0])
    box = ([2.1, 0.45, 0.15], [0.8, 0.5, 0.2], [-0.3, 0.2, 0.9], [0.4, 0.3, 0.25])
    objs = [w[0], _plane("pane red", *pane, red), w[2], _sphere("on the wall", [2.4, Y[0] + 0.25, 0.3], 0.25, red),
            _box("box red", *box, red), w[1], _plane("pane green", *pane, green), w[3],
            _box("in the wall", [2.7, Y[1] + 0.25, 0.4], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.5, 0.6, 0.6], green),
            _box("box green", *box, green), w[4], _sphere("on the floor", [1.8, -0.45, Z[0] + 0.25], 0.25, green),
            _box("on the floor", [2.7, -0.9, Z[0] + 0.2], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.4, 0.4, 0.4], red), w[5]]
    objs += _spheres(rs, ["s%d" % k for k in range(3)])
    return _write(out_dir, "twins", HEAD + TWO_LIGHTS + "world_objects:\n" + "".join(objs),
                  camera_text(1, 3, width, height))


def no_spheres(out_dir, width=48, height=27):
    """The room and a dozen boxes, no sphere at all: no hierarchy (bvh_root == BVH_NONE)."""
    rs = np.random.RandomState(47)
    objs = walls(rs, {"back": _texture("rails_synth.png", 1.0, 1.0, 0.02, 0.02)})
    objs += [_plain_box(rs, "b%02d" % k, kind=k % 2, glass=k % 4 == 3) for k in range(12)]
    order = rs.permutation(len(objs))
    return _write(out_dir, "no_spheres", HEAD + TWO_LIGHTS + "world_objects:\n" + "".join(objs[i] for i in order),
                  camera_text(2, 3, width, height))


def inside_box(out_dir, width=48, height=27):
    """No wall planes: one large box is the room, the camera inside it; a mirror box, a glass box and
    34 spheres (mirrors among them) inside."""
    rs = np.random.RandomState(53)
    room = _box("room", [6.0 * S, 0.0, 1.75 * S], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [16.0 * S, 6.5 * S, 12.0 * S],
                ([0.5, 0.45, 0.4], [0.03] * 3, [0.15] * 3, [0.0] * 3))
    objs = _spheres(rs, ["s%02d" % k for k in range(17)]) + [_plain_box(rs, "mirror", 1), room]
    objs += _spheres(rs, ["t%02d" % k for k in range(17)]) + [_plain_box(rs, "glass", glass=True)]
    return _write(out_dir, "inside_box", HEAD + TWO_LIGHTS + "world_objects:\n" + "".join(objs),
                  camera_text(1, 4, width, height))


def flush(out_dir, width=48, height=27):
    """36 large spheres behind the back wall, 0.002 to 0.004 of each in front of it, and nothing else in
    the room but two boxes: every box of the hierarchy begins a hair before the wall, and the wall's
    hit is the far bound the walk culls them against.  The caps are 0.2 wide: they win pixels."""
    rs = np.random.RandomState(59)
    objs = walls(rs) + [_plain_box(rs, "b0"), _plain_box(rs, "b1", 1)]
    for k in range(36):
        r = rs.uniform(1.5, 2.5)
        c = [X[1] + r - rs.uniform(0.002, 0.004), S * (-5.0 + 2.0 * (k % 6)) + rs.uniform(-0.1, 0.1),
             S * (-1.0 + 0.9 * (k // 6)) + rs.uniform(-0.05, 0.05)]
        objs.append(_sphere("s%02d" % k, c, r, make_scenes.material(rs, k % 3)))
    order = rs.permutation(len(objs))
    return _write(out_dir, "flush", HEAD + TWO_LIGHTS + "world_objects:\n" + "".join(objs[i] for i in order),
                  camera_text(1, 3, width, height))


# cover_stacks: the target is the ground's point under the light (0, 0, 10) of radius 2, lifted by the
# plane's delta; the partial covers are test_gpu_queries._six_cover_world's: sphere k at height z = 1 + k,
# radius 0.06 z, 0.03 z off the axis, wholly inside the light's cone (0.2 z there): cover 0.09 each, no acos.
STACK_LIGHT = (0.0, 0.0, 10.0, 2.0)
STACK_ORDERS = ("spheres_first", "box_plane_first", "alternating", "uncovered")
STACK_FILLERS = (0, 40, 120)


def _stack_parts(n):
    grey = ([0.5] * 3, [0.05] * 3, [0.3] * 3, [0.0] * 3)
    sph = [_sphere("c%d" % k, (0.03 * (1.0 + k) * np.cos(k), 0.03 * (1.0 + k) * np.sin(k), 1.0 + k), 0.06 * (1.0 + k), grey)
           for k in range(n)]
    lid = _box("lid", [0.0, 0.0, 7.5], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [3.0, 0.2, 3.0], grey)
    sheet = _plane("sheet", [0.0, 0.0, 8.5], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], grey)
    aside = _box("aside", [6.0, 0.0, 3.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0], grey)
    beyond = _plane("beyond", [0.0, 0.0, 12.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], grey)
    return sph, lid, sheet, aside, beyond


def cover_stacks(order, fillers, out_dir):
    """One light over a ground plane; more than COVER_K covers between the ground's points near the
    origin and the light, in the YAML order `order`; `fillers` far spheres (test_raises._fillers) so
    that a hierarchy, its LDS stagings and the light buffer are in play.  The camera looks down at
    the origin through a narrow retina: its 12 x 8 pixels' hits lie within 0.1 of it."""
    import test_raises as tr
    ground = _plane("ground", [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0],
                    ([0.6] * 3, [0.05] * 3, [0.3] * 3, [0.0] * 3))
    if order == "uncovered":                       # six partial covers, a plane and a box that cover nothing
        sph, lid, sheet, aside, beyond = _stack_parts(6)
        objs = [sph[0], beyond, sph[1], sph[2], aside, sph[3], sph[4], ground, sph[5]]
    else:
        sph, lid, sheet, aside, beyond = _stack_parts(5)
        objs = {"spheres_first": sph + [lid, sheet, ground],
                "box_plane_first": [lid, sheet] + sph + [ground],
                "alternating": [sph[0], lid, sph[1], ground, sph[2], sheet, sph[3], sph[4]]}[order]
    text = (HEAD + "lights:\n" + _light("L", STACK_LIGHT[:3], STACK_LIGHT[3], [0.5, 0.5, 0.5], 1.0, 1.0)
            + "world_objects:\n" + "".join(objs) + tr._fillers(fillers))
    cam = camera_text(1, 2, 12, 8, position=(0.0, -3.0, 1.5), front=(0.0, 3.0, -1.5), retina=(0.0002, 0.00015), pre=1, mx=1)
    return _write(out_dir, "stack_%s_%d" % (order, fillers), text, cam)


def stack_targets():
    """Explicit targets on the ground around the origin (the plane's delta above it), for World#lit_area."""
    return np.array([[x, y, 1e-5] for x in (-0.015, 0.0, 0.01) for y in (-0.01, 0.0, 0.015)])


HAND_MADE = {"sphere_runs": sphere_runs, "twins": twins, "no_spheres": no_spheres, "inside_box": inside_box,
             "flush": flush}
WORLDS = tuple("room%d" % k for k in range(len(ROOMS))) + tuple(HAND_MADE)


def world(name, out_dir, width=48, height=27):
    """(world.yml, camera.yml) of a world of WORLDS."""
    if name.startswith("room"):
        return make_room(int(name[4:]), out_dir, width, height)
    return HAND_MADE[name](out_dir, width, height)


def sha(paths):
    """sha256 (16 hex digits) of a world's files, the textures directory written as "<textures>"."""
    h = hashlib.sha256()
    for p in paths:
        with open(p) as f:
            h.update(f.read().replace(TEXTURES, "<textures>").encode())
    return h.hexdigest()[:16]


def yaml_runs(world_yml):
    """The number of type changes in the YAML's object list plus one."""
    from raytracing_rb_amd import config
    kinds = [o["type"] for o in config.load_yaml(world_yml)["world_objects"]]
    return 1 + sum(a != b for a, b in zip(kinds, kinds[1:]))


# ---------------------------------------------------------------- the oracle's account of a world
def _ray_row(ray):
    return ray.front.to_a() + ray.position.to_a()


@functools.lru_cache(maxsize=None)
def first_hits(world_yml, camera_yml, sample=0):
    """By oracle/rt_ref.py over the lens rays of `sample` with aperture_radius 0 (no libm call in them):
    rays [H, W, 6], ids [H, W, 3] and geom [H, W, 10] as tests/test_gpu_first_hit.py's expected(), and
    per pixel the winner's and the runner-up's (distance, object index) as `order` [H, W, 2, 2]
    (-1, inf where there is none), with World#intersect's own answer checked against the winner."""
    from oracle import rt_ref
    from oracle.rb_vec3 import RtxError
    from test_gpu_first_hit import _normal_only
    wd, cam = rt_ref.load_scene(world_yml, camera_yml, seed=1, overrides={"aperture_radius": 0.0})
    H, W = cam.height, cam.width
    rays = np.zeros((H, W, 6))
    ids = np.full((H, W, 3), -1, np.int32)
    geom = np.zeros((H, W, 10))
    order = np.full((H, W, 2, 2), np.inf)
    order[..., 1] = -1
    for y in range(H):
        for x in range(W):
            ray = cam.lens_func(x, y, sample)
            rays[y, x] = _ray_row(ray)
            found = []
            for k, o in enumerate(wd.objects):
                res = o.intersect(ray)
                if res and res[0] is not None:
                    d = ray.distance(res[0])
                    if d < wd.max_distance:
                        found.append((d, k, res))
            found.sort(key=lambda t: t[:2])
            for j, (d, k, _) in enumerate(found[:2]):
                order[y, x, j] = (d, k)
            if not found:
                geom[y, x, 0] = wd.max_distance
                continue
            d, k, (inter, direction, delta, data) = found[0]
            obj = wd.objects[k]
            ids[y, x] = (k, 0 if direction == "in" else 1, -1 if data is None else data)
            try:
                n = obj.intersect_parameters(ray, inter, direction, delta, data)[0]
            except RtxError:
                n = _normal_only(obj, ray, inter, direction, data)
            try:
                n = n.normalize().to_a()
            except RtxError:
                n = [0.0, 0.0, 0.0]
            a = obj.diffuse_rate
            if obj.texture is not None and not isinstance(obj, rt_ref.Box):
                try:
                    a = a * obj.texture.color(*obj.get_uv(inter))
                except RtxError:
                    a = rt_ref.Vec3(0.0, 0.0, 0.0)
            geom[y, x] = [d] + inter.to_a() + n + a.to_a()
    kinds = [type(o).__name__ for o in wd.objects]
    for a in (rays, ids, geom, order):
        a.setflags(write=False)
    return {"rays": rays, "ids": ids, "geom": geom, "order": order, "kinds": kinds, "max_distance": float(wd.max_distance)}


def hit_counts(fh):
    """What test_mixed_scenes.py's conditions are about, from first_hits()."""
    kinds = np.array(fh["kinds"])
    win, second = fh["order"][..., 0, 1].astype(int), fh["order"][..., 1, 1].astype(int)
    hit, two = win >= 0, second >= 0
    gap = np.where(two, fh["order"][..., 1, 0], 0.0) - np.where(two, fh["order"][..., 0, 0], 0.0)
    kw = np.where(hit, kinds[np.maximum(win, 0)], "none")
    ks = np.where(two, kinds[np.maximum(second, 0)], "none")
    out = {"rays": int(hit.size), "misses": int((~hit).sum())}
    for k in ("Sphere", "Plane", "Box"):
        out["first_" + k.lower()] = int((kw == k).sum())
    out["sphere_before_near_surface"] = int(((kw == "Sphere") & (ks != "Sphere") & two & (gap <= NEAR)).sum())
    tie = two & (gap == 0)
    out["ties_plane_plane"] = int((tie & (kw == "Plane") & (ks == "Plane")).sum())
    out["ties_box_box"] = int((tie & (kw == "Box") & (ks == "Box")).sum())
    out["near_ties_between_kinds"] = int((two & (kw != ks) & (gap <= 1e-9)).sum())
    return out


def near_rays(fh, limit=64):
    """The lens rays of first_hits() whose runner-up lies within NEAR of the winner: ties first."""
    two = fh["order"][..., 1, 1] >= 0
    gap = np.where(two, fh["order"][..., 1, 0] - np.where(two, fh["order"][..., 0, 0], 0.0), np.inf).reshape(-1)
    idx = np.argsort(gap, kind="stable")
    idx = idx[gap[idx] <= NEAR][:limit]
    return np.ascontiguousarray(fh["rays"].reshape(-1, 6)[idx])


def cap_rays(world_yml, origin=(0.0, 0.0, 0.0)):
    """One ray per small sphere (radius <= 0.16: the rooms' shallow caps among them) from `origin` at the point
    of the sphere nearest to it: where a cap shows, the surface it is sunk into lies a hair behind that point."""
    from raytracing_rb_amd import config
    o = np.array(origin, float)
    out = []
    for it in config.load_yaml(world_yml)["world_objects"]:
        p = it["properties"]
        if it["type"] == "Sphere" and float(p["radius"]) <= 0.16:
            c = np.array([float(t) for t in p["center"]])
            out.append(list(c - o) + list(o))
    return np.array(out, float).reshape(-1, 6)


class CoverCount:
    """World#lit_area (world.rb:62-69) of an rt_ref world with the same arithmetic, counting per call the
    non-zero covers and their kinds: `calls`, `long` (more than COVER_K covers) and `mixed` (long, and of
    at least two kinds)."""

    def __init__(self, world):
        self.world, self.calls, self.long, self.mixed, self.last = world, 0, 0, 0, ()

    def __enter__(self):
        wd = self.world

        def lit_area(target, light_pos, radius):
            total_area, kinds = 1, []
            for obj in wd.objects:
                c = obj.cover_area(light_pos, radius, target)
                total_area -= c
                if c != 0:
                    kinds.append(type(obj).__name__)
            self.calls += 1
            self.last = tuple(kinds)
            if len(kinds) > COVER_K:
                self.long += 1
                self.mixed += len(set(kinds)) >= 2
            return max(total_area, 0)
        wd.lit_area = lit_area
        return self

    def __exit__(self, *exc):
        del self.world.lit_area


def python_frame(world_yml, camera_yml, seed):
    """(frame, status, CoverCount) of rt_ref's render, pixel by pixel."""
    from oracle import rt_ref
    from oracle.rb_vec3 import RtxError
    wd, cam = rt_ref.load_scene(world_yml, camera_yml, seed=seed)
    codes = {"zero_vec": 1, "color_gt1": 2, "domain": 3}
    py = np.zeros((cam.height, cam.width, 3))
    st = np.zeros((cam.height, cam.width), np.int32)
    with CoverCount(wd) as cc:
        for x in range(cam.width):
            for y in range(cam.height):
                try:
                    py[y, x] = cam.render_at(x, y).to_a()
                except RtxError as e:
                    st[y, x] = codes[e.kind]
    return py, st, cc


SEED = 5                           # the render seed of every mixed world
TINY = (12, 8)                     # the size at which rt_ref renders them (test_oracle.py's)


def host_runs(exe, world_yml):
    """n_runs of the host scene build (tools/scene_dump.cpp, compiled by plan_scenes.build_tool)."""
    import subprocess
    p = subprocess.run([exe, world_yml], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout, p.stderr)
    return int([ln.split()[2] for ln in p.stdout.splitlines() if ln.startswith("scalar n_runs ")][0])


def cover_row(cc):
    return dict(shadow_queries=cc.calls, long_cover_lists=cc.long, long_mixed=cc.mixed)


def stack_area(world_yml, camera_yml):
    """rt_ref's lit_area of stack_targets() under STACK_LIGHT, and the CoverCount of those calls."""
    from oracle import rt_ref
    from oracle.rb_vec3 import Vec3
    wd = rt_ref.load_scene(world_yml, camera_yml)[0]
    with CoverCount(wd) as cc:
        area = [float(wd.lit_area(Vec3(*[float(v) for v in t]), Vec3(*STACK_LIGHT[:3]), STACK_LIGHT[3])) for t in stack_targets()]
    return np.array(area), cc


def fixture(out_dir):
    """tests/golden/mixed_scenes.json: per world its files' hash, its YAML run count, the launch plan
    the host build predicts (plan_scenes.host_plans), hit_counts() at 48 x 27 and the cover counts of
    rt_ref's TINY render; per stack its hash, plan, the cover counts of rt_ref's render and of
    stack_targets(), and the areas there (their float's repr)."""
    import plan_scenes
    exe = plan_scenes.build_tool(out_dir)
    out = {"worlds": {}, "stacks": {}}
    for name in WORLDS:
        w, c = world(name, out_dir)
        row = {"sha": sha((w, c)), "runs": yaml_runs(w), "plan": plan_scenes.host_plans(exe, [w])[0][0]}
        assert host_runs(exe, w) == row["runs"]
        row.update(hit_counts(first_hits(w, c)))
        _, st, cc = python_frame(*world(name, out_dir, *TINY), SEED)
        row.update(raising=int((st != 0).sum()), **cover_row(cc))
        out["worlds"][name] = row
    for order in STACK_ORDERS:
        for fillers in STACK_FILLERS:
            w, c = cover_stacks(order, fillers, out_dir)
            row = {"sha": sha((w, c)), "runs": yaml_runs(w), "plan": plan_scenes.host_plans(exe, [w])[0][0]}
            if fillers == 0:
                _, st, cc = python_frame(w, c, SEED)
                area, tc = stack_area(w, c)
                row.update(raising=int((st != 0).sum()), **cover_row(cc))
                row.update(targets_long=tc.long, targets_mixed=tc.mixed, area=[repr(float(a)) for a in area])
            out["stacks"]["%s_%d" % (order, fillers)] = row
    return out


if __name__ == "__main__":
    import json
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        fx = fixture(d)
    with open(os.path.join(ROOT, "tests", "golden", "mixed_scenes.json"), "w") as f:
        f.write("{\n" + ",\n".join("\"%s\": {\n%s\n}" % (part, ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v))
                                                                          for k, v in fx[part].items()))
                                   for part in ("worlds", "stacks")) + "\n}\n")
    for part in ("worlds", "stacks"):
        for k, v in fx[part].items():
            print(k, v)
