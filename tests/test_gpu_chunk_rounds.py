"""Chunk rounds of the bounce levels (option lv_round): the
static chunks of a level launch belong to a workgroup, whose waves claim them
from a counter in LDS, instead of to a wave.  Which wave runs which chunk
changes no bit: every ray writes its record at its dense index and the tree
reduction does not depend on the visiting order, so every frame here must be
identical to the lanes engine's (engine 0), for the per-wave schedule (0), for
rounds shorter than, equal to and longer than a workgroup's waves, and for the
longest round the option takes.

The mapping itself is checked on the host (test_sched_rounds.py)."""

import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, SCENES

pytestmark = pytest.mark.gpu

ROUNDS = (0, 1, 3, 8, 32, 4096)


def _scene(world, camera, **ov):
    from raytracing_rb_amd import config
    return config.load_scene(os.path.join(SCENES, world), os.path.join(SCENES, camera), camera_overrides=ov)


def _renderer(sd, cd, engine, **opts):
    from raytracing_rb_amd.runtime import Renderer
    r = Renderer(sd, cd, device=0)
    r.set_option("engine", engine)
    for k, v in opts.items():
        r.set_option(k, v)
    return r


def _same(a, b):
    """Bit-identical frames (also -0.0 vs 0.0 and NaN payloads)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


_LANES = {}


def _lanes(world, camera, ov, seed):
    """The lanes engine's frame of a scene: rendered once, shared, never written."""
    key = (world, camera, tuple(sorted(ov.items())), seed)
    if key not in _LANES:
        sd, cd = _scene(world, camera, **ov)
        r = _renderer(sd, cd, 0)
        fb = r.render(seed=seed)
        r.close()
        fb.setflags(write=False)
        _LANES[key] = (sd, cd, fb)
    return _LANES[key]


def _every_round_same(world, camera, ov, seed, opts, after=None):
    sd, cd, lanes = _lanes(world, camera, ov, seed)
    r = _renderer(sd, cd, 1, **opts)
    for rnd in ROUNDS:
        r.set_option("lv_round", rnd)
        assert r.get_option("lv_round") == rnd
        assert _same(r.render(seed=seed), lanes), (rnd, opts)
        if after:
            after(r, rnd)
    r.close()


def _no_overflow(r, rnd):
    st = r.level_stats()
    assert st["redo"] == 0 and st["dropped"] == 0, (rnd, st)


@pytest.mark.parametrize("ov", [
    dict(width=8, height=8, pre_sample_times=1),                              # one chunk: fewer chunks than waves
    dict(width=33, height=19, trace_depth=0),
    dict(width=33, height=19, trace_depth=1),
    dict(width=33, height=19, monte_carlo_diffusion_times=3, trace_depth=4),
])
def test_rounds_small_frames_and_depths(gpu, ov):
    _every_round_same("mix_world.yml", "mix_camera.yml", ov, 3, {}, _no_overflow)


def test_rounds_c2_hit_ring_crosses_claims(gpu):
    """C2 (the hierarchy and the full hit ring in LDS, k_level_c): hits parked
    in a wave's ring come from whichever chunks the wave claimed."""
    _every_round_same("c2_world.yml", "c2_camera.yml", dict(width=160, height=90), 3, {}, _no_overflow)


C2_SMALL = dict(width=120, height=70)


@pytest.mark.parametrize("opts", [
    dict(lv_static=37),                                  # rounds over the first 37 %, then the sharded global claims
    dict(lv_static=0),                                   # no static part: the first draw of every wave ends it
    dict(lv_grid_div=2),                                 # other numbers of workgroups
    dict(lv_grid_div=8),
    dict(lv_compact=0),                                  # k_level (no hit ring)
    dict(lv_split=1),                                    # k_lv_trace / k_lv_shadow / k_lv_shade: 256-thread blocks, 4 waves
    dict(lv_split=1, lv_static=37),
    dict(lv_sort=1, lv_sort_from=1),                     # binned levels (the chunks in bin order)
    dict(lv_streams=2),                                  # two parts at once, each with its own launches
    dict(lv_streams=1),
], ids=lambda o: "-".join("%s=%d" % kv for kv in o.items()))
def test_rounds_with_every_level_mode(gpu, opts):
    _every_round_same("c2_world.yml", "c2_camera.yml", C2_SMALL, 5, opts)


def test_rounds_batches_overflow_and_re_render(gpu):
    """Many batches with staging that overflows: the overflowing samples are
    re-rendered by the lanes engine, whichever wave found the slice full."""
    def redo(r, rnd):
        assert r.level_stats()["redo"] > 0, rnd
    _every_round_same("c2_world.yml", "c2_camera.yml", C2_SMALL, 5,
                      dict(lv_batch=1000, lv_stage_pct=5, lv_floor=0), redo)


@pytest.mark.parametrize("src", [1, 3])
def test_rounds_sphere_modes_without_staging(gpu, src):
    """Sphere records by scalar loads (no staging barrier of their own: the
    counter's barrier is the schedule's) and the plain staged hierarchy."""
    _every_round_same("c2_world.yml", "c2_camera.yml", C2_SMALL, 5, dict(sphere_src=src))
    _every_round_same("c2_world.yml", "c2_camera.yml", C2_SMALL, 5, dict(sphere_src=src, bvh=0))


def test_rounds_c4_golden_quantized_leaves(gpu):
    """C4 (nodes and 16-bit leaf records in LDS beside the compact ring, the
    tightest LDS layout; half of its chunks static): the golden frame's camera."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_scenes
    make_scenes.ensure_c4()
    z = np.load(os.path.join(GOLDEN, "frame_c4_48x27.npz"))
    ov = eval(str(z["overrides"]), {})
    _every_round_same(str(z["world"]), str(z["camera"]), ov, int(z["seed"]), dict(sphere_src=4))


def test_round_option_validated(gpu):
    from raytracing_rb_amd import _abi
    from raytracing_rb_amd.runtime import RtxError
    sd, cd = _scene("c2_world.yml", "c2_camera.yml", width=32, height=18)
    r = _renderer(sd, cd, 1)
    assert r.get_option("lv_round") == -1                 # auto
    for v in (-2, 4097, 1 << 20, -(1 << 40)):
        with pytest.raises(RtxError) as e:
            r.set_option("lv_round", v)
        assert e.value.status == _abi.RTX_EINVAL, v
    assert r.get_option("lv_round") == -1                 # a refused value changes nothing
    for v in (-1, 0, 1, 4096):
        r.set_option("lv_round", v)
        assert r.get_option("lv_round") == v
    r.close()
