"""What makes tests/test_gpu_deep_trees.py mean something, checked on the oracles
alone (no GPU): the worlds of tests/deep_scenes.py really fill the stacks.

Per case (trace_depth D, monte_carlo_diffusion_times pt) of deep_scenes.CASES:

* some sample's pending siblings (rt_map_tree.max_pending's discipline, the
  engines') peak at (D - 1) * (1 + pt) = need - 1, the most any tree can: D - 1
  for pt 0, and above the next smaller stack bucket for every pt > 0 case but
  (17, 1), where need - 1 = 32 is that bucket's size exactly: no tree tells a
  32-entry stack from the 64 entries that camera gets, so (18, 1) stands beside
  it (34 pending);
* the C oracle's frame at D differs from the frame at D - 1 by >= 1e-4 at some
  pixel, 100 times the GPU tests' max |diff| bound: the deepest level cannot
  hide inside the tolerance;
* no sample raises;
* the recorded values of tests/golden/deep_trees.json (make_deep_trees.py) are
  what the C oracle counts today, and the Python oracle's trees of sampled
  pixels, expanded by rt_map_tree, count the same.

monte_carlo_diffusion_times 0 (world_object.rb:78 divides diffuse_rate by
0.0, a plain C division in the reference): the two oracles agree bit for bit
at depths 9 and 64 on pixels whose trees have unlit hits.
"""
import numpy as np
import pytest

import deep_scenes
import rt_map_tree as T
from oracle.c_oracle import Oracle

FIX = deep_scenes.fixture()
ROWS = deep_scenes.rows()
PIXELS = ((0, 0), (4, 3), (7, 5), (3, 2))


def test_the_fixture_has_every_row_and_no_other():
    assert sorted(FIX) == sorted(r[0] for r in ROWS)
    assert {(5, 0), (6, 0), (8, 0), (9, 0), (16, 0), (17, 0), (20, 0), (21, 0), (32, 0), (33, 0), (64, 0), (16, 1), (17, 1),
            (32, 1), (5, 14), (4, 15)} <= set(deep_scenes.CASES)


@pytest.mark.parametrize("name,depth,pt,w,h", ROWS, ids=[r[0] for r in ROWS])
def test_recorded_values_and_the_peak(oracle_lib, tmp_path, name, depth, pt, w, h):
    got = deep_scenes.measure(depth, pt, tmp_path, w, h)          # (asserts that no sample raises)
    row = FIX[name]
    assert {k: row[k] for k in got} == got, name
    assert (row["depth"], row["pt"], row["width"], row["height"], row["seed"]) == (depth, pt, w, h, deep_scenes.SEED)
    assert len(row["rays_per_level"]) == depth and row["rays_per_level"][0] == w * h and row["rays_per_level"][-1] > 0
    need = deep_scenes.need(depth, pt)
    assert row["max_pending"] == need - 1 and row["samples_at_max"] >= 1
    if pt == 0:
        assert row["max_pending"] == depth - 1
    elif (depth, pt) != (17, 1):                                  # (see the module's text)
        smaller = {16: 8, 32: 16, 64: 32}[deep_scenes.bucket(need)]
        assert row["max_pending"] > smaller, (name, smaller)
    else:
        assert row["max_pending"] == 32 and deep_scenes.bucket(need) == 64 and FIX["d18_pt1"]["max_pending"] > 32


@pytest.mark.parametrize("depth,pt", deep_scenes.CASES, ids=[deep_scenes.case_name(*c) for c in deep_scenes.CASES])
def test_the_deepest_level_shows_in_the_frame(oracle_lib, tmp_path, depth, pt):
    frames = []
    for d in (depth, depth - 1):
        frame, st, rc = Oracle(*deep_scenes.load(d, pt, tmp_path)).render(seed=deep_scenes.SEED)
        assert rc == 0 and not st.any()
        frames.append(frame)
    diff = np.abs(frames[0] - frames[1]).max()
    print("%s: max |frame(D) - frame(D - 1)| %.3e" % (deep_scenes.case_name(depth, pt), diff))
    assert diff >= 1e-4


def _python_trees(depth, pt, out_dir, pixels):
    """The Python oracle's trees of the pixels' sample 0, expanded level by level."""
    from oracle import rt_ref
    world, cam = rt_ref.load_scene(*deep_scenes.make(depth, pt, out_dir), seed=deep_scenes.SEED)
    rays = np.array([(lambda r: r.front.to_a() + r.position.to_a())(cam.lens_func(x, y, 0)) for x, y in pixels])
    roots = T.level0(rays, np.array([(x, y, 0) for x, y in pixels], np.int32), depth)
    levels = T.expand(roots, T.oracle_rt_map(cam.ray_tracer))
    assert not any(k for _, out in levels for k in out["raised"])
    return cam, levels


@pytest.mark.parametrize("depth,pt,pixels", [(9, 0, PIXELS), (17, 0, PIXELS[:2]), (17, 1, PIXELS), (18, 1, PIXELS[:2]),
                                             (4, 15, PIXELS[:1])])
def test_max_pending_of_the_python_oracles_trees(oracle_lib, tmp_path, depth, pt, pixels):
    """rt_map_tree.max_pending over the Python oracle's expanded trees against the C oracle's count
    (rt_oracle.c rto_tree_stats: live entries of trace_sync's Array, less the one held), pixel by pixel,
    and the live rays per level."""
    _, levels = _python_trees(depth, pt, tmp_path, pixels)
    peak, live = T.max_pending(levels)
    pend, per_level, st, rc = Oracle(*deep_scenes.load(depth, pt, tmp_path)).tree_stats(pixels, seed=deep_scenes.SEED)
    assert rc == 0
    assert peak.tolist() == pend.tolist()
    assert len(per_level) == depth and live[:depth].tolist() == per_level.tolist()
    assert not live[depth:].any()                                 # (the level of remaining depth 0: nothing passes)
    assert peak.max() <= deep_scenes.need(depth, pt) - 1
    sums, gt1 = T.tree_sums(levels)
    assert not gt1.any()
    ref, st, rc = Oracle(*deep_scenes.load(depth, pt, tmp_path)).render_pixels(pixels, seed=deep_scenes.SEED)
    assert np.array_equal(sums.view(np.uint64), ref.view(np.uint64))


def test_max_pending_holds_the_last_live_child():
    """Hand-made levels: a root with three children of which the last is dead (the second is held, one
    stacked), the held one with two live children (one more stacked), a dead root."""
    def level(att, depth):
        n = len(att)
        return {"rays": np.zeros((n, 6)), "att": np.array(att, float).reshape(n, 3), "keys": np.full((n, 4), depth, np.int32),
                "paths": np.ones(n, np.uint64)}

    def out(nch):
        return {"n_children": np.array(nch, np.int32)}
    one, dead = [1.0, 1.0, 1.0], [5e-5, 5e-5, 5e-5]            # |dead| = 8.7e-5 < 1e-4
    levels = [(level([one, dead], 3), out([3, 0])),
              (level([one, one, dead], 2), out([1, 2, 0])),
              (level([one, one, one], 1), out([0, 0, 0]))]
    peak, live = T.max_pending(levels)
    assert peak.tolist() == [2, 0] and live.tolist() == [1, 2, 3]


@pytest.mark.parametrize("depth", [9, 64])
def test_pt0_python_and_c_oracles_agree(oracle_lib, tmp_path, depth):
    """monte_carlo_diffusion_times 0: WorldObject#path_tracing divides by 0.0 at every unlit hit
    (infinity, used by a loop that runs zero times) and raises nothing."""
    from oracle import rt_ref
    world, cam = rt_ref.load_scene(*deep_scenes.make(depth, 0, tmp_path), seed=deep_scenes.SEED)
    unlit = []
    path_tracing = rt_ref.WorldObject.path_tracing

    def spy(self, intersection, n, pt_times, draw):
        unlit.append(pt_times)
        return path_tracing(self, intersection, n, pt_times, draw)
    rt_ref.WorldObject.path_tracing = spy
    try:
        py = np.array([cam.render_at(x, y).to_a() for x, y in PIXELS])
    finally:
        rt_ref.WorldObject.path_tracing = path_tracing
    assert len(unlit) >= 4 * (depth // 2 - 1) and set(unlit) == {0}        # the chain's :out hits
    ref, st, rc = Oracle(*deep_scenes.load(depth, 0, tmp_path)).render_pixels(PIXELS, seed=deep_scenes.SEED)
    assert rc == 0 and not st.any()
    assert np.isfinite(py).all()
    assert np.array_equal(py.view(np.uint64), ref.view(np.uint64))


LIGHT_CASES = ((32, 32), (32, 20), (31, 31))                                   # test_gpu_deep_trees.py's


@pytest.mark.parametrize("n_light,k", LIGHT_CASES)
def test_the_many_light_worlds(oracle_lib, tmp_path, n_light, k):
    """No sample raises (k leaves of att * colour * rate / k a central ray), and the central pixel's roots are
    highlight nodes of exactly k leaves, by the Python oracle."""
    import plan_scenes
    from oracle import rt_ref
    from raytracing_rb_amd import config
    w, c = plan_scenes._write(tmp_path, "hl_%d_%d" % (n_light, k), plan_scenes.multi_highlight_text(n_light, k),
                              plan_scenes.camera_text(width=16, height=10))
    frame, st, rc = Oracle(*config.load_scene(w, c)).render(seed=1)
    assert rc == 0 and not st.any() and frame.max() <= 1.0
    world, cam = rt_ref.load_scene(w, c)
    assert len(world.lights) == n_light
    for j in (0, 1):                                              # pixel (8, 5) of 16 x 10 looks down the axis
        children, leaves = cam.ray_tracer.rt_map((cam.lens_func(8, 5, j), cam.trace_depth, rt_ref.Vec3(1.0, 1.0, 1.0), 1), 8, 5, j)
        assert not children and len(leaves) == k
