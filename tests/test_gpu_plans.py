"""Parity over the launch plans of the bounce-level engine (csrc/rtx_plan.h).

Every row of tests/golden/level_plans.json is a seeded world (plan_scenes.py) whose
own size sends the default options down one branch of the plan: sphere mode, hit
ring, light buffer and raise gates in LDS or not, raise-check variant, claim
counter placed or not.  Per row, at 48 x 27 with 2 / 3 samples:

* the launcher's own record of what it launched (read-only option lv_plan_last)
  is the committed plan, the one the host tool predicted (test_level_plans.py);
* the default frame against the C oracle with test_gpu_fuzz.py's bounds: RMS <= 1e-4
  per channel, max |diff| <= 1e-6 (no row raises: test_level_plans.py);
* the lanes engine, the ordered linear walk, the split phases, no hit ring, no
  light buffer and exact_raises 0 give the default frame's bits.
* the engine's other entry, rtx_trace_device under "trace_engine" 1 with 64 lens rays,
  records the same plan and returns the lanes engine's colours and statuses.

The 513-sphere world with its last sphere hidden renders the 512-sphere world's
bits; rtx_lit_area and rtx_rt_map (LMAX = 17 / 32) against the Python oracle on
the rows of 17 and 32 lights; worlds whose central rays fire 3, 9 and 32
highlights at once."""
import numpy as np
import pytest

import plan_scenes
from test_level_plans import HL_CASES, TABLE

pytestmark = pytest.mark.gpu

VARIANTS = (("lanes", {"engine": 0}), ("linear", {"bvh": 0}), ("split", {"lv_split": 1}), ("no ring", {"lv_compact": 0}),
            ("no light buffer", {"lbuf": 0}), ("no raise check", {"exact_raises": 0}))
ROWS = {r["name"]: r for r in TABLE}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _render(sd, cd, seed, opts=()):
    from raytracing_rb_amd.runtime import Renderer
    r = Renderer(sd, cd, device=0)
    for k, v in dict(opts).items():
        r.set_option(k, v)
    frame = r.render(seed=seed)
    plan, stats = r.get_option("lv_plan_last"), r.level_stats()
    r.close()
    return frame, plan, stats


def _against_the_oracle(frame, sd, cd, seed, where):
    from oracle.c_oracle import Oracle
    ref, st, rc = Oracle(sd, cd).render(seed=seed)
    assert rc == 0 and not st.any(), where
    d = frame - ref
    rms = np.sqrt((d.reshape(-1, 3) ** 2).mean(axis=0))
    print("%s: RMS %s max |diff| %.3e bit-exact pixels %.4f" % (where, rms, np.abs(d).max(), np.mean(np.all(frame == ref, axis=2))))
    assert (rms <= 1e-4).all(), (where, rms)
    assert np.abs(d).max() <= 1e-6, (where, np.abs(d).max())


@pytest.mark.parametrize("name", list(ROWS))
def test_row_renders_its_plan(gpu, tmp_path, name):
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    row = ROWS[name]
    sd, cd = config.load_scene(*plan_scenes.row_world(row, tmp_path))
    assert (cd.width, cd.height, cd.trace_depth, cd.monte_carlo_diffusion_times) == (48, 27, row["depth"], row["pt"])
    r = Renderer(sd, cd, device=0)                 # one upload; every variant sets its option and puts it back
    frame = r.render(seed=plan_scenes.SEED)
    plan = r.get_option("lv_plan_last")
    assert plan == row["plan"], (plan_scenes.unpack_plan(plan), plan_scenes.unpack_plan(row["plan"]))
    _against_the_oracle(frame, sd, cd, plan_scenes.SEED, name)
    for label, opts in VARIANTS:
        default = {k: r.get_option(k) for k in opts}
        for k, v in opts.items():
            r.set_option(k, v)
        other = r.render(seed=plan_scenes.SEED)
        oplan = r.get_option("lv_plan_last")
        for k, v in default.items():
            r.set_option(k, v)
        assert np.array_equal(_bits(other), _bits(frame)), (name, label)
        if label == "split" and row["n_light"] <= 16:
            assert oplan == -1, (name, label)              # no fused level launch ran
        elif label == "no ring":
            assert plan_scenes.unpack_plan(oplan)["ring"] == 0, (name, label)
    assert np.array_equal(_bits(r.render(seed=plan_scenes.SEED)), _bits(frame)) and r.get_option("lv_plan_last") == plan
    r.close()


@pytest.mark.parametrize("name", list(ROWS))
def test_row_traces_its_plan(gpu, tmp_path, name):
    """The engine's other entry goes through the same selection: the 64 lens rays of an 8 x 8 camera
    (pre 1) through rtx_trace_device under "trace_engine" 1 launch the row's committed plan, and
    their colours and statuses are the lanes engine's ("trace_engine" 0) bit for bit."""
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    row = ROWS[name]
    sd, cd = config.load_scene(*plan_scenes.row_world(row, tmp_path),
                               camera_overrides={"width": 8, "height": 8, "pre_sample_times": 1})
    r = Renderer(sd, cd, device=0)
    rays = np.ascontiguousarray(r.lens_rays(sample=0, seed=plan_scenes.SEED).reshape(-1, 6))
    keys = np.array([(x, y, 0) for y in range(8) for x in range(8)], np.int32)
    assert rays.shape == (64, 6)
    r.set_option("trace_engine", 1)
    rgb, st = r.trace(rays, keys, seed=plan_scenes.SEED, check=False)
    plan = r.get_option("lv_plan_last")
    assert r.get_option("trace_engine_last") == 1
    assert plan == row["plan"], (plan_scenes.unpack_plan(plan), plan_scenes.unpack_plan(row["plan"]))
    r.set_option("trace_engine", 0)
    lanes_rgb, lanes_st = r.trace(rays, keys, seed=plan_scenes.SEED, check=False)
    assert r.get_option("trace_engine_last") == 0 and r.get_option("lv_plan_last") == -1   # no level launch ran
    r.close()
    assert np.array_equal(st, lanes_st), name
    assert np.array_equal(_bits(rgb), _bits(lanes_rgb)), name


def test_the_hidden_sphere_changes_no_bit(gpu, tmp_path):
    """The 513-sphere world takes the host build's other side (global buffers, per-sphere raise lists);
    with its 513th sphere under the ground behind the camera the picture is the 512-sphere world's."""
    from raytracing_rb_amd import config
    frames = {}
    for key, (row, hide) in {"512": (ROWS["lds_512_l17"], False), "513 hidden": (ROWS["lds_513_l17"], True)}.items():
        sd, cd = config.load_scene(*plan_scenes.row_world(row, tmp_path, hide_last=hide))
        frames[key], plan, _ = _render(sd, cd, plan_scenes.SEED)
        assert plan_scenes.unpack_plan(plan)["mode"] == plan_scenes.unpack_plan(row["plan"])["mode"]
    assert np.array_equal(_bits(frames["512"]), _bits(frames["513 hidden"]))


# ---------------------------------------------------------------- queries with 17 and 32 lights
QUERY_ROWS = ("ldsx_32_l17", "ldsx_32_l32", "lds_513_l17", "lds_536_l32")
PIXELS = [(x, y) for y in (15, 18, 21, 25) for x in (5, 17, 29, 41)]       # below the horizon: every ray hits


def _query_oracle(name, out_dir):
    """By the Python oracle: the 16 pixels' lens rays of sample 0, their first-hit
    targets with expected_lit_area, and the root rt_map call of each ray."""
    import rt_map_tree as T
    from oracle import rt_ref
    from test_gpu_queries import expected_lit_area
    from test_gpu_rt_map import _LocalLightsAcos
    world, cam = rt_ref.load_scene(*plan_scenes.row_world(ROWS[name], out_dir))
    rays = np.array([(lambda r: r.front.to_a() + r.position.to_a())(cam.lens_func(x, y, 0)) for x, y in PIXELS])
    keys = np.array([(x, y, 0) for x, y in PIXELS], np.int32)
    level = T.level0(rays, keys, cam.trace_depth)
    index = {id(o): i for i, o in enumerate(world.objects)}
    notes, targets = [], []

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
    for i in range(len(rays)):
        obj, inter, _, delta, _ = world.intersect(T.oracle_item(level, i)[0][0])
        assert obj is not None
        targets.append((inter + delta).to_a())
    targets = np.array(targets)
    return level, out, targets, expected_lit_area(world, targets), cam.ray_tracer.pt_times


@pytest.mark.parametrize("name", QUERY_ROWS)
def test_lit_area_and_rt_map_with_many_lights(gpu, tmp_path_factory, name):
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    from test_gpu_queries import assert_lit_area
    from test_gpu_rt_map import OUTS, TOL
    out_dir = tmp_path_factory.mktemp("q_" + name)
    level, exp, targets, exp_area, pt = _query_oracle(name, out_dir)
    nl = ROWS[name]["n_light"]
    sd, cd = config.load_scene(*plan_scenes.row_world(ROWS[name], out_dir))
    r = Renderer(sd, cd, device=0)
    # rtx_lit_area, lights = NULL: L = n_light entries per target
    area, color, status = r.lit_area(targets, check=False)
    assert area.shape == (16, nl) and color.shape == (16, nl, 3)
    assert np.array_equal(status != 0, exp_area[3])
    assert_lit_area(area, color, exp_area, name)
    a = exp_area[0]
    assert (a == 0).any() and (a == 1).any()                  # shadowed and lit entries
    # rtx_rt_map of the same pixels' lens rays: LMAX = n_light
    got = r.rt_map(level["rays"], level["keys"], att=level["att"], paths=level["paths"], check=False)
    r.close()
    assert got["leaves"].shape == (16, nl, 3)
    info = np.stack([got[k] for k in OUTS[:6]], axis=1)
    bad = np.nonzero((info != exp["info"]).any(axis=1))[0]
    assert len(bad) == 0, (name, bad[:5].tolist(), info[bad[0]].tolist(), exp["info"][bad[0]].tolist())
    assert np.array_equal(got["child_paths"], exp["child_paths"])
    ch, ech = got["children"], exp["children"]
    assert np.array_equal(_bits(ch[..., 3:]), _bits(ech[..., 3:]))          # position, attenuation
    exact = exp["child_paths"] % np.uint64(pt + 3) <= 1                     # unused slots and reflections
    assert np.array_equal(_bits(ch[..., :3])[exact], _bits(ech[..., :3])[exact])
    assert np.abs(ch[..., :3] - ech[..., :3]).max() <= TOL
    # leaves: bit for bit but for the local-lighting leaf of a node whose local_lights called Math.acos
    kind = exp["info"][:, 1]
    loose = (kind == 3) & (exp["acos"] > 0)
    lf, elf = got["leaves"], exp["leaves"]
    assert np.array_equal(_bits(lf)[~loose], _bits(elf)[~loose])
    assert np.abs(lf - elf).max() <= TOL
    assert (kind == 3).sum() >= 8                             # lit hits: local_lights over all the lights


# ---------------------------------------------------------------- several highlights on one ray
@pytest.mark.parametrize("n_light,k", HL_CASES)
def test_k_highlights_on_one_ray(gpu, tmp_path, n_light, k):
    import rt_map_tree as T
    from oracle import rt_ref
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    w, c = plan_scenes.make_multi_highlight(n_light, k, tmp_path)
    sd, cd = config.load_scene(w, c)
    frame, plan, stats = _render(sd, cd, 1)
    assert plan >= 0 and stats["redo"] == 0
    _against_the_oracle(frame, sd, cd, 1, "highlights %d of %d" % (k, n_light))
    lanes, _, _ = _render(sd, cd, 1, {"engine": 0})
    assert np.array_equal(_bits(lanes), _bits(frame))
    # a deferred-check list of 64 entries overflows: those samples are re-rendered by the lanes engine
    small, _, stats = _render(sd, cd, 1, {"lv_hl_cap": 64})
    assert np.array_equal(_bits(small), _bits(frame))
    assert stats["redo"] > 0, stats
    # the central rays' root rt_map: a highlight node of k leaves, the oracle's bits (no libm call in them)
    world, cam = rt_ref.load_scene(w, c)
    px = ((23, 13), (24, 13), (23, 12), (24, 14), (0, 0))
    rays = np.array([(lambda q: q.front.to_a() + q.position.to_a())(cam.lens_func(x, y, 0)) for x, y in px])
    level = T.level0(rays, np.array([(x, y, 0) for x, y in px], np.int32), cam.trace_depth)
    exp = T.oracle_rt_map(cam.ray_tracer)(level)
    r = Renderer(sd, cd, device=0)
    got = r.rt_map(level["rays"], level["keys"], att=level["att"], paths=level["paths"])
    r.close()
    assert got["kind"][:4].tolist() == [1] * 4 and got["n_leaves"][:4].tolist() == [k] * 4
    assert got["n_children"][:4].tolist() == [0] * 4 and got["kind"][4] != 1
    assert np.array_equal(got["n_leaves"], exp["n_leaves"]) and np.array_equal(got["n_children"], exp["n_children"])
    assert np.array_equal(_bits(got["leaves"][:4, :k]), _bits(exp["leaves"][:4, :k]))
