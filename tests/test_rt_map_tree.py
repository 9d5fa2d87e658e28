"""tests/rt_map_tree.py proved on the CPU before it judges the GPU
(tests/test_gpu_rt_map.py): trees expanded level by level through
rt_ref.RayTracer.rt_map and summed in trace_sync's order equal rt_ref.trace_sync
bit for bit (oracle/rt_ref.py, the restatement of ray_tracer.rb:16-164)."""

import os
import sys

import numpy as np
import pytest

from conftest import scene_paths

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def oracle_roots(cam, w, h):
    """rays [n, 6], keys [n, 3] of every pre sample of a w x h frame, by rt_ref.Camera.lens_func."""
    rays, keys = [], []
    for y in range(h):
        for x in range(w):
            for j in range(cam.pre_sample_times):
                r = cam.lens_func(x, y, j)
                rays.append(r.front.to_a() + r.position.to_a())
                keys.append((x, y, j))
    return np.array(rays, np.float64), np.array(keys, np.int32)


@pytest.mark.parametrize("name,w,h,live", [("c2", 16, 9, 2130), ("mix", 12, 7, 16771)])
def test_helper_equals_trace_sync(name, w, h, live):
    import rt_map_tree as T
    from oracle import rt_ref
    from oracle.rb_vec3 import RtxError
    world, cam = rt_ref.load_scene(*scene_paths(name), overrides=dict(width=w, height=h))
    rays, keys = oracle_roots(cam, w, h)
    levels = T.expand(T.level0(rays, keys, cam.trace_depth), T.oracle_rt_map(cam.ray_tracer))
    assert len(levels) == cam.trace_depth + 1                     # the last level: the dead children alone
    assert not any(k for _, out in levels for k in out["raised"])
    alive = sum(int(T.live_mask(lv).sum()) for lv, _ in levels)
    total = sum(len(lv["rays"]) for lv, _ in levels)
    print(name, "nodes", total, "live", alive)
    assert alive == live and total > alive
    sums, gt1 = T.tree_sums(levels)
    for i in range(len(rays)):
        x, y, j = (int(v) for v in keys[i])
        try:
            want = cam.ray_tracer.trace_sync(x, y, cam.lens_func(x, y, j), j).to_a()
        except RtxError as e:                                     # rt_reduce's raise: the helper flags the same tree
            assert e.kind == "color_gt1" and gt1[i], (i, e.kind)
            continue
        assert not gt1[i]
        assert np.array_equal(sums[i].view(np.uint64), np.array(want, np.float64).view(np.uint64)), (i, sums[i], want)
