"""Parity on worlds of many planes and boxes in mixed YAML order
(tests/mixed_scenes.py; what is in them is asserted on the CPU by
tests/test_mixed_scenes.py): closed rooms where every ray has a far bound,
spheres sunk into walls and box faces, twins, boxes in general position, a box
as the room, sphere runs of 1 to 7 at unaligned records, more covers of mixed
kinds on one shadow ray than the cover list holds.

Per world, one Renderer whose options are set and put back: the default frame
against the C oracle within test_gpu_plans.py's bounds (RMS <= 1e-4 per
channel, max |diff| <= 1e-6), the launcher's plan the committed one, and the
same bits from the lanes engine, the ordered linear walk, the hierarchy forced
with every sphere source, the split phases, both other rings, no light buffer
and exact_raises 0.  Then the queries: rtx_first_hit and rtx_intersect bit for
bit against oracle/rt_ref.py (tests/test_gpu_first_hit.py's rule: aperture 0,
no libm call, no tolerance), rtx_lit_area on the cover stacks, rtx_rt_map one
level deep, rtx_trace_device against the lanes engine, rtx_count_work against
the oracle's counters."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

import mixed_scenes as M
import plan_scenes

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "mixed_scenes.json")) as _f:
    FIXTURE = json.load(_f)

VARIANTS = ((("lanes", {"engine": 0}), ("linear", {"bvh": 0}), ("hierarchy", {"bvh": 2}))
            + tuple(("hierarchy, sphere_src %d" % k, {"bvh": 2, "sphere_src": k}) for k in range(5))
            + (("split", {"lv_split": 1}), ("no ring", {"lv_compact": 0}), ("compact ring", {"lv_compact": 2}),
               ("no light buffer", {"lbuf": 0}), ("no raise check", {"exact_raises": 0})))
WALKS = ((("bvh", 0),), (("bvh", 2),), (("bvh", 2), ("sphere_src", 1)))       # test_gpu_queries.py's: LIN, BVH_LDS, BVH_GLOBAL
STACKS = [(o, f) for o in M.STACK_ORDERS for f in M.STACK_FILLERS]


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("mixed"))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _renderer(w, c, **ov):
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    sd, cd = config.load_scene(w, c, camera_overrides=ov)
    return Renderer(sd, cd, device=0), sd, cd


class _Options:
    """Set a renderer's options and put them back."""

    def __init__(self, r, opts):
        self.r, self.opts = r, dict(opts)

    def __enter__(self):
        self.was = {k: self.r.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.r.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.was.items():
            self.r.set_option(k, v)


def _frame_and_variants(w, c, plan, where):
    from test_gpu_plans import _against_the_oracle
    r, sd, cd = _renderer(w, c)
    assert cd.width <= 48 and cd.height <= 27
    frame = r.render(seed=M.SEED)
    got = r.get_option("lv_plan_last")
    assert got == plan, (where, plan_scenes.unpack_plan(got), plan_scenes.unpack_plan(plan))
    _against_the_oracle(frame, sd, cd, M.SEED, where)
    for label, opts in VARIANTS:
        with _Options(r, opts):
            other = r.render(seed=M.SEED)
        bad = np.argwhere((_bits(other) != _bits(frame)).any(axis=2))
        assert len(bad) == 0, (where, label, len(bad), bad[:5].tolist())
    assert np.array_equal(_bits(r.render(seed=M.SEED)), _bits(frame)) and r.get_option("lv_plan_last") == plan
    r.close()
    return frame


@pytest.mark.parametrize("name", M.WORLDS)
def test_frame_against_the_oracle_and_every_walk(gpu, out_dir, name):
    _frame_and_variants(*M.world(name, out_dir), FIXTURE["worlds"][name]["plan"], name)


@pytest.mark.parametrize("order,fillers", STACKS)
def test_stack_frames(gpu, out_dir, order, fillers):
    """The 12 x 8 pixels that look at the stacks' targets: inside the level kernels the light-buffer walk's
    `after` passes answer them.  Under the sheet all is shadow: a dropped cover would light a pixel."""
    where = "%s_%d" % (order, fillers)
    frame = _frame_and_variants(*M.cover_stacks(order, fillers, out_dir), FIXTURE["stacks"][where]["plan"], where)
    assert (frame > 0).all() if order == "uncovered" else (frame == 0).all()


# ---------------------------------------------------------------- queries
def _inside_rays(world_yml, seed=3):
    """Two rays from the centre of every box, at random: they start inside it."""
    from raytracing_rb_amd import config
    rng = np.random.default_rng(seed)
    out = []
    for it in config.load_yaml(world_yml)["world_objects"]:
        if it["type"] == "Box":
            for _ in range(2):
                out.append(list(rng.normal(size=3)) + [float(t) for t in it["properties"]["point"]])
    return np.array(out, float).reshape(-1, 6)


def _ray_table(name, w, fh):
    """The explicit rays of a world: the lens rays whose runner-up lies within 0.05 of the winner (the ties
    first), a ray at every shallow cap, rays from inside the boxes; for twins, rays from inside the tangent
    spheres at their points of tangency and along the twin box's faces."""
    rays = [M.near_rays(fh), M.cap_rays(w), _inside_rays(w)]
    if name == "twins":
        rays.append(np.array([[0.0, -1.0, 0.0, 2.4, M.Y[0] + 0.25, 0.3], [0.0, 0.0, -1.0, 1.8, -0.45, M.Z[0] + 0.25],
                              [0.0, 0.0, -1.0, 2.7, -0.9, 0.5], [0.0, 1.0, 0.0, 2.7, 0.0, 0.4]]))
    return np.ascontiguousarray(np.concatenate([a for a in rays if len(a)]))


@pytest.mark.parametrize("name", M.WORLDS)
def test_first_hit_and_intersect(gpu, out_dir, name):
    from oracle import rt_ref
    from test_gpu_first_hit import _assert_equal, _buffers
    from test_gpu_queries import _buffers as _ibuffers, expected_intersect
    w, c = M.world(name, out_dir)
    fh = M.first_hits(w, c)
    r, sd, cd = _renderer(w, c, aperture_radius=0.0)
    assert np.array_equal(_bits(r.lens_rays(sample=0)), _bits(fh["rays"]))
    _assert_equal(_buffers(r.first_hit(sample=0)), fh)
    rays = _ray_table(name, w, fh)
    ids, geom, nearest = expected_intersect(rt_ref.load_scene(w, c)[0], rays)
    ties = [i for i, ks in enumerate(nearest) if len(ks) > 1]
    print(name, len(rays), "rays,", int((ids[:, 0] >= 0).sum()), "hits,", len(ties), "ties")
    if name == "twins":
        assert len(ties) >= 10
    for opts in WALKS:
        with _Options(r, opts):
            got_ids, got_geom = _ibuffers(r.intersect(rays))
        bad = np.nonzero((got_ids != ids).any(axis=1))[0]
        assert len(bad) == 0, (name, opts, bad[:5].tolist(), got_ids[bad[0]], ids[bad[0]])
        bad = np.nonzero((_bits(got_geom) != _bits(geom)).any(axis=1))[0]
        assert len(bad) == 0, (name, opts, bad[:5].tolist(), got_geom[bad[0]].tolist(), geom[bad[0]].tolist())
        for i in ties:                                            # the lower YAML index wins
            assert got_ids[i, 0] == min(nearest[i])
    r.close()


@pytest.mark.parametrize("order,fillers", STACKS)
def test_lit_area_on_the_stacks(gpu, out_dir, order, fillers):
    """A covered target gives exactly 0.0 whatever the order of the covers; an uncovered one the oracle's
    bits (no cover of these calls acos: test_mixed_scenes.py), decided by the ordered sum of six covers."""
    from test_gpu_queries import TOL
    w, c = M.cover_stacks(order, fillers, out_dir)
    T = M.stack_targets()
    exp = np.array([float(a) for a in FIXTURE["stacks"]["%s_0" % order]["area"]])
    lights = np.array([M.STACK_LIGHT] * len(T), np.float64)
    r, sd, cd = _renderer(w, c)
    for opts in ((),) + WALKS:
        with _Options(r, opts):
            a_scene, color, st_scene = r.lit_area(T)
            a_expl, _, st_expl = r.lit_area(T, lights=lights)
        assert not st_scene.any() and not st_expl.any()
        for area in (a_scene, a_expl):
            assert area.shape == (len(T), 1)
            assert np.array_equal(_bits(area[:, 0]), _bits(exp)), (order, fillers, opts, area[:, 0].tolist(), exp.tolist())
        if order == "uncovered":
            assert np.abs(color[:, 0] - (0.5 * exp * exp)[:, None]).max() <= TOL
        else:
            assert (exp == 0).all() and not np.signbit(a_scene).any() and (color == 0).all()
    r.close()


def _rt_map_oracle(w, c, ov):
    """test_gpu_plans.py's _query_oracle over a whole small frame: the root rt_map call of every lens ray of
    sample 0 by the Python oracle, with the expected info rows and local_lights' acos calls."""
    import rt_map_tree as T
    from oracle import rt_ref
    from test_gpu_rt_map import _LocalLightsAcos
    world, cam = rt_ref.load_scene(w, c, seed=M.SEED, overrides=dict(ov))
    px = [(x, y) for y in range(cam.height) for x in range(cam.width)]
    rays = np.array([M._ray_row(cam.lens_func(x, y, 0)) for x, y in px])
    level = T.level0(rays, np.array([(x, y, 0) for x, y in px], np.int32), cam.trace_depth)
    index = {id(o): i for i, o in enumerate(world.objects)}
    notes = []

    def on_item(level, i, call):
        with _LocalLightsAcos(world) as cnt:
            children, leaves = call()
        hit = (-1, -1)
        if children:
            obj, _, direction, _, _ = world.intersect(T.oracle_item(level, i)[0][0])
            hit = (index[id(obj)], 0 if direction == "in" else 1)
        notes.append((cnt.n,) + hit)
        return children, leaves
    out = T.oracle_rt_map(cam.ray_tracer, on_item)(level)
    assert not any(out["raised"])
    nt = np.array(notes, np.int64)
    nch, nlf = out["n_children"], out["n_leaves"]
    kind = np.where(nch > 0, np.where(nlf > 0, 3, 4), np.where(nlf > 0, 1, 2))
    out["acos"] = nt[:, 0]
    out["info"] = np.stack([np.zeros(len(nt), np.int64), kind, nt[:, 1], nch, nlf, nt[:, 2]], axis=1).astype(np.int32)
    return level, out, cam.ray_tracer.pt_times, [type(o).__name__ for o in world.objects]


@pytest.mark.parametrize("name", ("room1", "inside_box"))
def test_rt_map_one_level_deep(gpu, out_dir, name):
    """Children, leaves and statuses of the root call of a 16 x 9 frame's lens rays, with test_gpu_plans.py's
    rule: bit for bit but for refraction and path-tracing fronts and the leaves whose local_lights called acos."""
    from test_gpu_rt_map import OUTS, TOL
    ov = dict(width=16, height=9)
    w, c = M.world(name, out_dir)
    level, exp, pt, kinds = _rt_map_oracle(w, c, ov)
    r, sd, cd = _renderer(w, c, **ov)
    got = r.rt_map(level["rays"], level["keys"], att=level["att"], paths=level["paths"], seed=M.SEED, check=False)
    r.close()
    info = np.stack([got[k] for k in OUTS[:6]], axis=1)
    bad = np.nonzero((info != exp["info"]).any(axis=1))[0]
    assert len(bad) == 0, (name, bad[:5].tolist(), info[bad[0]].tolist(), exp["info"][bad[0]].tolist())
    assert np.array_equal(got["child_paths"], exp["child_paths"])
    ch, ech = got["children"], exp["children"]
    assert np.array_equal(_bits(ch[..., 3:]), _bits(ech[..., 3:]))          # position, attenuation
    exact = exp["child_paths"] % np.uint64(pt + 3) <= 1                     # unused slots and reflections
    assert np.array_equal(_bits(ch[..., :3])[exact], _bits(ech[..., :3])[exact])
    assert np.abs(ch[..., :3] - ech[..., :3]).max() <= TOL
    kind = exp["info"][:, 1]
    loose = (kind == 3) & (exp["acos"] > 0)
    lf, elf = got["leaves"], exp["leaves"]
    assert np.array_equal(_bits(lf)[~loose], _bits(elf)[~loose])
    assert np.abs(lf - elf).max() <= TOL
    hit = exp["info"][:, 2]
    seen = {kinds[k] for k in hit[hit >= 0]}
    assert seen == ({"Sphere", "Plane", "Box"} if name == "room1" else {"Sphere", "Box"}), seen
    assert (kind == 3).sum() >= 16 and (kind == 4).sum() >= 4 and (~loose & (kind == 3)).sum() >= 4


@pytest.mark.parametrize("name", ("room1", "room2", "inside_box"))
def test_trace_device_equals_the_lanes_engine(gpu, out_dir, name):
    """The frame's lens rays of sample 0 as an explicit batch through the bounce levels: the committed plan,
    the lanes engine's colours and statuses, and the oracle's colours within the frame's bounds."""
    from oracle.c_oracle import Oracle
    from test_gpu_trace_levels import _lens, _same, _trace
    w, c = M.world(name, out_dir)
    r, sd, cd = _renderer(w, c)
    rays, keys = _lens(r, seed=M.SEED)
    lv = _trace(r, rays, keys, 1, seed=M.SEED)
    assert r.get_option("lv_plan_last") == FIXTURE["worlds"][name]["plan"]
    lanes = _trace(r, rays, keys, 0, seed=M.SEED)
    r.close()
    assert not lv[1].any() and _same(lv, lanes), name
    ref, ost, rc = Oracle(sd, cd).trace(rays, keys, seed=M.SEED)
    assert rc == 0 and not ost.any()
    d = lv[0] - ref
    assert np.abs(d).max() <= 1e-6 and (np.sqrt((d ** 2).mean(axis=0)) <= 1e-4).all()


def test_work_counters(gpu, out_dir):
    """rtx_count_work against the oracle's brute-force event counts on the 40-sphere room, within
    test_gpu_parity.py's margin; the plane and box counters are a large part of the work here."""
    from oracle.c_oracle import Oracle
    from raytracing_rb_amd._abi import COUNTER_NAMES
    r, sd, cd = _renderer(*M.world("room1", out_dir))
    got = r.count_work()
    r.close()
    _, _, _, cnt = Oracle(sd, cd).render(counts=True)
    ref = dict(zip(COUNTER_NAMES, [int(v) for v in cnt[:len(COUNTER_NAMES)]]))
    print(ref)
    for k in ("plane_tests", "box_tests", "cover_plane", "cover_box", "cover_sphere", "sphere_hits"):
        assert ref[k] > 1000, (k, ref[k])
    for k in ref:
        assert abs(got[k] - ref[k]) <= max(2, 1e-4 * ref[k]), (k, got[k], ref[k])
