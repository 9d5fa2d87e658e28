"""Deep ray trees, monte_carlo_diffusion_times 0 and the engines' limits against the
C oracle (tests/deep_scenes.py; the conditions that make these renders fill the
stacks are held on the oracles alone by tests/test_deep_trees.py).

Per case (trace_depth, pt) of deep_scenes.CASES, 8 x 6 pixels of one sample:

* the default render against the C oracle under test_gpu_plans' bounds (RMS <=
  1e-4 per channel, max |diff| <= 1e-6);
* engine 0, bvh 0 and bvh 2 give the default frame's bits;
* rtx_level_stats: no sample re-rendered, and the rays per tree level are the
  oracle's (tests/golden/deep_trees.json), level by level from level 1 on (level
  0 counts the items of the padded 8 x 8 tiles): a subtree dropped by
  an undersized walk stack can hide in a colour tolerance, not in this count
  (the count is taken where the levels are built, so it is the reduction's
  frame against the oracle's that shows a subtree the reduction skipped: the
  row worlds' frames move by >= 1e-4 with their deepest level alone);
* rtx_count_work, which runs the lanes engine, counts the oracle's rays.

The ray stack's LDS half and the crossover to its global half (lds_stack),
force_stack, a context whose stack regrows, the refusals at need > 64, worlds
of 32 lights, the most a scene holds, where every light or only some fire on
one ray, postpone and a median-split hierarchy.
"""
import ctypes as C

import numpy as np
import pytest

import deep_scenes
import plan_scenes
from test_gpu_plans import _against_the_oracle, _bits

pytestmark = pytest.mark.gpu

FIX = deep_scenes.fixture()
SEED = deep_scenes.SEED
IDS = [deep_scenes.case_name(*c) for c in deep_scenes.CASES]


def _renderer(depth, pt, out_dir, width=8, height=6):
    from raytracing_rb_amd.runtime import Renderer
    sd, cd = deep_scenes.load(depth, pt, out_dir, width, height)
    return Renderer(sd, cd, device=0), sd, cd


def _with(r, opts, seed=SEED):
    """A render with the options set, then put back."""
    default = {k: r.get_option(k) for k in opts}
    for k, v in opts.items():
        r.set_option(k, v)
    try:
        return r.render(seed=seed)
    finally:
        for k, v in default.items():
            r.set_option(k, v)


def _paths_fit_32_bits(depth, pt):
    return (pt + 3) ** depth <= 2 ** 32


def _check_levels(r, row, where):
    """rtx_level_stats against the oracle's rays per level.  Level 0 of the statistics is the batch's items,
    the padding of the frame's 8 x 8 tiles included; from level 1 on they are rays that passed rt_map's cutoff."""
    stats = r.level_stats()
    assert stats["redo"] == 0 and stats["dropped"] == 0, (where, stats)
    items = ((row["width"] + 7) // 8) * ((row["height"] + 7) // 8) * 64
    assert row["rays_per_level"][0] == row["width"] * row["height"]
    assert stats["rays"] == [items] + row["rays_per_level"][1:], (where, stats["rays"], row["rays_per_level"])


@pytest.mark.parametrize("depth,pt", deep_scenes.CASES, ids=IDS)
def test_case_against_the_oracle(gpu, tmp_path, depth, pt):
    name = deep_scenes.case_name(depth, pt)
    row = FIX[name]
    r, sd, cd = _renderer(depth, pt, tmp_path)
    levels = pt <= 14
    assert r.get_option("engine_effective") == (1 if levels else 0) and r.engine() == ("levels" if levels else "lanes")
    assert r.get_option("lv_ray_bytes_effective") == (80 if _paths_fit_32_bits(depth, pt) else 96)
    frame = r.render(seed=SEED)
    if levels:
        _check_levels(r, row, name)
    else:
        assert r.level_stats()["rays"] == []                      # the lanes engine keeps no level statistics
    _against_the_oracle(frame, sd, cd, SEED, name)
    for label, opts in (("lanes", {"engine": 0}), ("linear", {"bvh": 0}), ("hierarchy", {"bvh": 2})):
        assert np.array_equal(_bits(_with(r, opts)), _bits(frame)), (name, label)
    assert r.count_work(seed=SEED)["rays"] == row["rays"], name
    r.close()


def test_the_ray_record_edges():
    """3^20 < 2^32 < 3^21 and 4^16 = 2^32 < 4^17: the cases on both sides of the 80 | 96 byte record."""
    assert [_paths_fit_32_bits(*c) for c in ((20, 0), (21, 0), (16, 1), (17, 1))] == [True, False, True, False]


@pytest.mark.parametrize("depth,pt", deep_scenes.WIDE, ids=[deep_scenes.case_name(*c) for c in deep_scenes.WIDE])
def test_level_options_on_deep_trees(gpu, tmp_path, depth, pt):
    """16 x 10: two 8 x 8 tiles a row, so lv_streams 2 has two parts and lv_fin_grid's blocks loop over tiles."""
    name = deep_scenes.case_name(depth, pt) + "_16x10"
    r, sd, cd = _renderer(depth, pt, tmp_path, 16, 10)
    frame = r.render(seed=SEED)
    _check_levels(r, FIX[name], name)
    _against_the_oracle(frame, sd, cd, SEED, name)
    for opts in ({"lv_streams": 1}, {"lv_split": 1}, {"lv_compact": 0}, {"lv_fin_grid": 2}):
        assert np.array_equal(_bits(_with(r, opts)), _bits(frame)), (name, opts)
        _check_levels(r, FIX[name], (name, opts))
    # level buffers far smaller than a level: the samples without room are re-rendered by the lanes engine
    small = {"lv_stage_pct": 5, "lv_floor": 0}
    default = {k: r.get_option(k) for k in small}
    for k, v in small.items():
        r.set_option(k, v)
    other = r.render(seed=SEED)
    stats = r.level_stats()
    for k, v in default.items():
        r.set_option(k, v)
    assert stats["redo"] > 0, stats
    assert np.array_equal(_bits(other), _bits(frame)), (name, small)
    r.close()


# ---------------------------------------------------------------- the lanes engine's ray stack
@pytest.mark.parametrize("depth,pt", [(64, 0), (32, 1)], ids=["d64_pt0", "d32_pt1"])
def test_ray_stack_in_lds_and_global_memory(gpu, tmp_path, depth, pt):
    """lds_stack k: a lane's bottom k entries in LDS, the rest in its global region; these trees' 63 and 62
    pending entries cross from one half to the other at every k (-1: as many as fit)."""
    r, _, _ = _renderer(depth, pt, tmp_path)
    r.set_option("engine", 0)
    assert r.get_option("lds_stack") == 0
    base = r.render(seed=SEED)
    assert np.array_equal(_bits(_with(r, {"engine": 1})), _bits(base))
    for bvh in (0, 2):
        for k in (0, 1, 3, -1):
            assert np.array_equal(_bits(_with(r, {"bvh": bvh, "lds_stack": k})), _bits(base)), (bvh, k)
    r.close()


def test_force_stack(gpu, tmp_path):
    from raytracing_rb_amd.runtime import RtxError
    r, _, _ = _renderer(9, 0, tmp_path)                           # need 9: bucket 16
    frame = r.render(seed=SEED)
    for engine in (0, 1):
        r.set_option("engine", engine)
        for v in (16, 17, 64):
            assert np.array_equal(_bits(_with(r, {"force_stack": v})), _bits(frame)), (engine, v)
        for v in (1, 8):                                          # a bucket of 8 entries below the need of 9
            with pytest.raises(RtxError) as e:
                _with(r, {"force_stack": v})
            assert e.value.kind == "invalid" and "needs a ray stack of 9 entries" in str(e.value), str(e.value)
            with pytest.raises(RtxError) as e:
                r.set_option("force_stack", v)
                try:
                    r.render_at(4, 3, seed=SEED)
                finally:
                    r.set_option("force_stack", 0)
            assert e.value.kind == "invalid"
        assert np.array_equal(_bits(r.render(seed=SEED)), _bits(frame))
    for v in (-1, 65, 1 << 20):
        with pytest.raises(RtxError) as e:
            r.set_option("force_stack", v)
        assert e.value.kind == "invalid" and r.get_option("force_stack") == 0
    r.close()


def test_a_contexts_stack_regrows(gpu, tmp_path):
    """One context: a camera of need 5, then need 64 (its global stack regions are allocated anew), then 5."""
    fresh = {}
    for depth in (5, 64):
        r, _, _ = _renderer(depth, 0, tmp_path)
        r.set_option("engine", 0)
        fresh[depth] = r.render(seed=SEED)
        r.close()
    assert not np.array_equal(fresh[5], fresh[64])
    r, _, _ = _renderer(5, 0, tmp_path)
    r.set_option("engine", 0)
    for depth in (5, 64, 5, 64):
        r.set_camera(deep_scenes.load(depth, 0, tmp_path)[1])
        assert np.array_equal(_bits(r.render(seed=SEED)), _bits(fresh[depth])), depth
    r.close()


# ---------------------------------------------------------------- limits
@pytest.mark.parametrize("depth,pt,need", [(65, 0, 65), (33, 1, 65), (5, 15, 65), (64, 1, 127), (100, 0, 100)])
def test_a_stack_above_64_entries_is_refused(gpu, tmp_path, depth, pt, need):
    """need = 1 + (depth - 1) * (1 + pt) > 64: RTX_EINVAL from both engines, from render, render_at and trace.
    rtx_rt_map answers one call per item and sizes no stack: it is not refused."""
    from raytracing_rb_amd.runtime import Renderer, RtxError
    assert deep_scenes.need(depth, pt) == need > 64
    sd, cd = deep_scenes.load(depth, pt, tmp_path)
    r = Renderer(sd, cd, device=0)
    ray = np.array([[1.0, 0.01, 0.02, 0.0, 0.0, 0.0]])             # (front, position): just off the axis
    for engine in (1, 0):
        r.set_option("engine", engine)
        for call in (lambda: r.render(seed=SEED), lambda: r.render_at(4, 3, seed=SEED),
                     lambda: r.trace(ray, [[4, 3, 0]], seed=SEED), lambda: r.count_work(seed=SEED)):
            with pytest.raises(RtxError) as e:
                call()
            assert e.value.kind == "invalid" and "%d entries" % need in str(e.value), str(e.value)
        with pytest.raises(RtxError) as e:                        # force_stack cannot talk it into rendering
            _with(r, {"force_stack": 64})
        assert e.value.kind == "invalid"
    got = r.rt_map(ray, [[4, 3, 0, depth]], seed=SEED)
    assert got["status"].tolist() == [0] and got["n_children"].tolist() == [2 + pt]       # (an unlit hit in the shell worlds)
    r.close()


LIGHT_CASES = ((32, 32), (32, 20), (31, 31))                                   # lights, of them on the camera's axis


@pytest.mark.parametrize("n_light,k", LIGHT_CASES)
def test_many_lights_on_one_ray(gpu, tmp_path, n_light, k):
    """32 lights are the most a scene holds (rtx_scene_upload; the highlight loop keeps the fired lights in a
    32-bit mask), far below the 255 of levels_engine() and of a tree record's 8-bit leaf count.  k of them on
    the camera's axis fire on the central pixel's rays (plan_scenes.multi_highlight_text): k leaves, the
    oracle's bits; the frame against the oracle and the other engine."""
    import rt_map_tree as T
    from oracle import rt_ref
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    w, c = plan_scenes._write(tmp_path, "hl_%d_%d" % (n_light, k), plan_scenes.multi_highlight_text(n_light, k),
                              plan_scenes.camera_text(width=16, height=10))
    sd, cd = config.load_scene(w, c)
    r = Renderer(sd, cd, device=0)
    assert r.get_option("engine_effective") == 1
    frame = r.render(seed=1)
    stats = r.level_stats()
    assert stats["redo"] == 0 and stats["dropped"] == 0 and len(stats["rays"]) == cd.trace_depth, stats
    _against_the_oracle(frame, sd, cd, 1, "highlights %d of %d" % (k, n_light))
    assert np.array_equal(_bits(_with(r, {"engine": 0}, seed=1)), _bits(frame))
    world, cam = rt_ref.load_scene(w, c)
    px = ((8, 5, 0), (8, 5, 1), (7, 5, 0), (0, 0, 0))             # pixel (8, 5) of 16 x 10 looks down the axis
    rays = np.array([(lambda q: q.front.to_a() + q.position.to_a())(cam.lens_func(x, y, j)) for x, y, j in px])
    level = T.level0(rays, np.array(px, np.int32), cam.trace_depth)
    exp = T.oracle_rt_map(cam.ray_tracer)(level)
    got = r.rt_map(level["rays"], level["keys"], att=level["att"], paths=level["paths"])
    r.close()
    assert got["kind"].tolist()[:2] == [1, 1] and got["n_leaves"].tolist()[:2] == [k, k] and 1 not in got["kind"][2:]
    assert np.array_equal(got["n_leaves"], exp["n_leaves"]) and np.array_equal(got["n_children"], exp["n_children"])
    assert np.array_equal(_bits(got["leaves"][:2, :k]), _bits(exp["leaves"][:2, :k]))


def test_a_33rd_light_is_refused(gpu, tmp_path):
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer, RtxError
    w, c = plan_scenes._write(tmp_path, "hl_33", plan_scenes.multi_highlight_text(33, 33), plan_scenes.camera_text(width=16, height=10))
    with pytest.raises(RtxError) as e:
        Renderer(*config.load_scene(w, c), device=0)
    assert e.value.kind == "invalid" and "at most 32 lights" in str(e.value)


# ---------------------------------------------------------------- walk options
MID = dict(n_sphere=533, n_light=2, seed=plan_scenes.SEED, around=False, pt=1, depth=3)      # 84 hierarchy nodes


def test_postpone_and_the_median_hierarchy(gpu, tmp_path):
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    sd, cd = config.load_scene(*plan_scenes.row_world(MID, tmp_path))
    r = Renderer(sd, cd, device=0)
    frame = r.render(seed=plan_scenes.SEED)
    _against_the_oracle(frame, sd, cd, plan_scenes.SEED, "mid-size world")
    assert r.get_option("postpone") == -1 and r.get_option("bvh_sah") == 1
    for v in (0, 1, 16, 64):                                      # lanes engine: walks left in fewer lanes wait
        assert np.array_equal(_bits(_with(r, {"engine": 0, "postpone": v}, seed=plan_scenes.SEED)), _bits(frame)), v
    r.set_option("bvh_sah", 0)                                    # takes effect at the next upload
    r._check(r.lib.rtx_scene_upload(r.h, C.byref(sd.desc)))
    median = r.render(seed=plan_scenes.SEED)
    assert np.array_equal(_bits(median), _bits(frame))
    _against_the_oracle(median, sd, cd, plan_scenes.SEED, "mid-size world, median hierarchy")
    for opts in ({"engine": 0}, {"engine": 0, "postpone": 0}, {"bvh": 0}):
        assert np.array_equal(_bits(_with(r, opts, seed=plan_scenes.SEED)), _bits(frame)), opts
    r.close()
