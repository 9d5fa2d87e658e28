"""Frames and traced rays against the bits the parent commit's library rendered
(tests/golden/parent_bits_*.npz, written by tests/golden/make_parent_bits.py).

The level kernels' wave-uniform short cuts (a division by a uniform 1.0 skipped,
decode_item's tile indices on the scalar unit with shift and mask for a
power-of-two pre_sample_times, the light-buffer walk's own set-up with its
cheaper finiteness test, the packed raise band test) must change no bit.  The
lanes engine shares the changed functions, so comparing the two engines with
each other would miss a common mistake: both are compared, on uint64 views,
with frames stored before the change.  Every case is 64x36 or smaller.
"""

import copy
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, SCENES

pytestmark = pytest.mark.gpu

SEED = 7
SMALL = dict(width=33, height=19)

# name -> (world, lights kept (None: all), camera file, camera overrides, options)
FRAMES = {
    # the mix scene has two lights: the first alone (n_light == 1), and both (the division stays)
    "mix_one_light": ("mix", 1, "mix", dict(SMALL), {}),
    "mix_two_lights": ("mix", None, "mix", dict(SMALL), {}),
    "mix_one_light_pt1": ("mix", 1, "mix", dict(SMALL, monte_carlo_diffusion_times=1, trace_depth=4), {}),
    "mix_one_light_pt3": ("mix", 1, "mix", dict(SMALL, monte_carlo_diffusion_times=3, trace_depth=4), {}),
    "mix_two_lights_pt3": ("mix", None, "mix", dict(SMALL, monte_carlo_diffusion_times=3, trace_depth=4), {}),
    "mix_pre1": ("mix", 1, "mix", dict(SMALL, pre_sample_times=1, max_sample_times=1), {}),
    "mix_pre3": ("mix", 1, "mix", dict(SMALL, pre_sample_times=3, max_sample_times=3), {}),
    "mix_pre4": ("mix", 1, "mix", dict(SMALL, pre_sample_times=4, max_sample_times=4), {}),
    # max_sample_times above pre: pass 1's extra samples (variant_threshold 0: every pixel takes them)
    "mix_pre2_max5": ("mix", 1, "mix", dict(SMALL, pre_sample_times=2, max_sample_times=5, variant_threshold=0.0), {}),
    "mix_pre3_max7": ("mix", None, "mix", dict(SMALL, pre_sample_times=3, max_sample_times=7, variant_threshold=0.0),
                      {}),
    # C2 (one area light): the light-buffer walk, without and with the raise band test
    "c2_xr0": ("c2", None, "c2", dict(width=64, height=36), dict(exact_raises=0)),
    "c2_xr1": ("c2", None, "c2", dict(width=64, height=36), dict(exact_raises=1)),
    # C4: textures, 16-bit leaf records, per-sphere raise lists
    "c4": ("c4", None, "c4", dict(width=48, height=27), {}),
}
FRAME_FILES = {"mix": [n for n in FRAMES if n.startswith("mix_") and "_pre" not in n],
               "samples": [n for n in FRAMES if n.startswith("mix_pre")], "c2": ["c2_xr0", "c2_xr1"], "c4": ["c4"]}
TILES = ("mix", 1, "mix", dict(SMALL), {})          # 8-row tiles, rank 1 of 3 (row_to_y)
TILE_ROWS, TILE_RANK, TILE_NRANKS = 8, 1, 3


def _scene(world, lights, camera, ov):
    from raytracing_rb_amd import config
    if world == "c4":
        import sys
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import make_scenes
        make_scenes.ensure_c4()
    wpath = os.path.join(SCENES, "%s_world.yml" % world)
    wcfg = config.load_yaml(wpath)
    if lights is not None:
        wcfg = copy.deepcopy(wcfg)
        wcfg["lights"] = wcfg["lights"][:lights]
    ccfg = config.load_yaml(os.path.join(SCENES, "%s_camera.yml" % camera))
    ccfg.update(ov)
    return config.SceneDescriptor(wcfg, os.path.dirname(wpath)), config.build_camera(ccfg)


def _renderer(spec, engine):
    from raytracing_rb_amd.runtime import Renderer
    world, lights, camera, ov, opts = spec
    r = Renderer(*_scene(world, lights, camera, ov), device=0)
    r.set_option("engine", engine)
    for k, v in opts.items():
        r.set_option(k, v)
    return r


def render_frame(name, engine):
    r = _renderer(FRAMES[name], engine)
    fb = r.render(seed=SEED)
    r.close()
    return fb


def render_tiles(engine):
    import torch
    r = _renderer(TILES, engine)
    rows = r.rows_per_rank(TILE_ROWS, TILE_NRANKS)
    packed = torch.zeros((rows, r.width, 3), dtype=torch.float64, device="cuda:0")
    s = torch.cuda.current_stream()
    r.render_tiles_device(packed.data_ptr(), TILE_ROWS, TILE_RANK, TILE_NRANKS, seed=SEED, stream=s.cuda_stream)
    r.sync(s.cuda_stream)
    out = packed.cpu().numpy()
    r.close()
    return out


# rtx_trace rays (front, position) whose shadow and bounce walks the float32 set-up cannot
# serve or serves at its edge: zero components, a zero direction, non-finite origins
RAY_WORLDS = (("mix", 1), ("c2", None))
RAYS = np.array([
    [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, -1, 0, 0, 0], [0, 0, 1, 0, 0, 0], [-1, 0, 0, 0, 0, 0],
    [1, 1, 0, 0, 0, 0], [1, 0, -0.2, 0, 0, 0], [0, 1, -0.3, 0, 0, 0], [1, -0.0, -0.05, 0, 0, 0],
    [1, 1e-25, -0.2, 0, 0, 0], [1, 1e-300, -0.1, 0, 0, 0], [1e-30, 0, -1e-30, 0, 0, 0],
    [0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 2, 3],
    [1, 0, -0.2, np.inf, 0, 0], [1, 0, -0.2, 0, -np.inf, 0], [1, 0.1, -0.2, np.nan, 0, 0],
    [1, 0.1, -0.2, 0, 0, np.nan], [1, 0, 0, 1e300, 0, 0], [0, 0, -1, 0, 0, 1e38],
], np.float64)


def trace_rays(world, lights, engine):
    """(status int32 [n], colours [n, 3]): one ray per call, because rtx_trace fails the whole call on a raise."""
    from raytracing_rb_amd.runtime import Renderer, RtxError
    r = Renderer(*_scene(world, lights, world, dict(width=40, height=24)), device=0)
    r.set_option("engine", engine)
    status = np.zeros(len(RAYS), np.int32)
    out = np.zeros((len(RAYS), 3), np.float64)
    for k, ray in enumerate(RAYS):
        try:
            out[k] = r.trace(ray[None], [[k % 40, k % 24, 0]], seed=SEED)[0]
        except RtxError as e:
            status[k] = e.status
    r.close()
    return status, out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def parent():
    z = {}
    for f in list(FRAME_FILES) + ["rays"]:
        with np.load(os.path.join(GOLDEN, "parent_bits_%s.npz" % f)) as d:
            z.update({k: d[k] for k in d.files})
    return z


@pytest.mark.parametrize("engine", [1, 0])
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frame_has_the_parent_bits(gpu, parent, name, engine):
    fb = render_frame(name, engine)
    ref = parent[name]
    assert fb.shape == ref.shape
    bad = np.argwhere(_bits(fb) != _bits(ref))
    assert len(bad) == 0, "%d values differ, first at (y, x, c) = %s" % (len(bad), bad[0])


@pytest.mark.parametrize("engine", [1, 0])
def test_tile_share_has_the_parent_bits(gpu, parent, engine):
    got = render_tiles(engine)
    ref = parent["tiles_rank1of3"]
    assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref))


@pytest.mark.parametrize("engine", [1, 0])
@pytest.mark.parametrize("world,lights", RAY_WORLDS)
def test_degenerate_rays_have_the_parent_bits(gpu, parent, world, lights, engine):
    status, out = trace_rays(world, lights, engine)
    assert np.array_equal(status, parent["rays_%s_status" % world]), status
    ref = parent["rays_%s" % world]
    bad = np.argwhere(_bits(out) != _bits(ref))
    assert len(bad) == 0, "ray %d differs: %s vs %s" % (bad[0][0], out[bad[0][0]], ref[bad[0][0]])
