"""Parity off the origin pose (tests/fuzz_scenes.py pose / make_posed).

Every scenes/*camera*.yml and fuzz_scenes.make() put the camera at the origin
looking along +x with up = +z, unit and perpendicular bases, the geometry
within ~30 units and max_distance at 10000.  There lens_func's normalizes
(camera.rb:129-151) change no bit, max_distance never binds and the float32
culls run at one scene scale S.  The posed
scenes are the same fuzz scenes under p -> t + scale Q p with a random rotation,
scale 0.02 / 1 / 40, |t| up to 1e5 scale, non-unit and non-perpendicular
camera and object bases, and max_distance at 9 scale (inside the geometry) on
half of them.  tests/test_oracle.py checks on the CPU that the two restatements
agree on them and that they stay in view.

Bounds as in test_gpu_fuzz.py: the default engine against the live C oracle,
RMS <= 1e-4 per channel and max |diff| <= 1e-6; engines, walks and buffers
against each other bit for bit.
"""

import os
import re
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu

VARIANTS = (("levels", {}), ("lanes", {"engine": 0}), ("linear", {"bvh": 0}), ("hier", {"bvh": 2}),
            ("no light buffer", {"lbuf": 0}), ("no exact raises", {"exact_raises": 0}))


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _check_against_oracle(fb, ref):
    d = fb - ref
    rms = np.sqrt((d.reshape(-1, 3) ** 2).mean(axis=0))
    print("rms %s, max |diff| %.3e, bit-exact pixels %.4f" % (rms, np.abs(d).max(), np.mean(np.all(fb == ref, axis=-1))))
    assert (rms <= 1e-4).all(), rms
    assert np.abs(d).max() <= 1e-6, np.abs(d).max()


@pytest.mark.parametrize("k", range(12))
def test_posed_scene_matches_oracle(gpu, tmp_path, k):
    import fuzz_scenes
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer, RtxError
    from oracle.c_oracle import Oracle
    seed = fuzz_scenes.POSED_SEEDS[k]
    w, c = fuzz_scenes.make_posed(seed, tmp_path, 48, 27)
    sd, cd = config.load_scene(w, c)
    ref, st, rc = Oracle(sd, cd).render(seed=seed)
    print("posed seed %d: scale %g, offset %g, bind_distance %d, oracle status %d"
          % ((seed,) + fuzz_scenes.posed_parameters(seed) + (rc,)))
    frames = {}
    for name, opts in VARIANTS:
        if rc and "exact_raises" in opts:
            continue                      # without the check a raise may go unreported: compared where none is
        r = Renderer(sd, cd, device=0)
        for key, v in opts.items():
            r.set_option(key, v)
        if rc:
            # the first raise in render_sync order, as the oracle's
            with pytest.raises(RtxError) as e:
                r.render(seed=seed)
            m = re.search(r"pixel \((\d+),(\d+)\)", str(e.value))
            x, y = int(m.group(1)), int(m.group(2))
            first = min((x_ * cd.height + y_ for y_, x_ in zip(*np.nonzero(st))))
            assert (x, y) == (first // cd.height, first % cd.height), (name, str(e.value))
            assert e.value.status == rc, (name, str(e.value))
        else:
            frames[name] = r.render(seed=seed)
        r.close()
    if rc:
        return
    fb = frames["levels"]
    _check_against_oracle(fb, ref)
    for name, _ in VARIANTS[1:]:
        assert _same(frames[name], fb), name


@pytest.fixture(scope="module")
def c4_world():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_scenes
    return make_scenes.ensure_c4()


@pytest.mark.parametrize("offset", [30.0, 2000.0])
def test_c4_posed_matches_oracle(gpu, tmp_path, c4_world, offset):
    """4,096 spheres off the origin: 16-bit quantized leaves, the global light and
    raise buffers and binning of every level (sphere mode 6), against the live C
    oracle and bit for bit against the linear walk and sphere_src 2 and 4."""
    import fuzz_scenes
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    from oracle.c_oracle import Oracle
    w, c = fuzz_scenes.pose(c4_world, os.path.join(SCENES, "c4_camera.yml"), tmp_path, 4, 1.0, offset, False)
    ov = dict(width=32, height=18, pre_sample_times=2, max_sample_times=2, trace_depth=4)
    sd, cd = config.load_scene(w, c, camera_overrides=ov)
    t0 = time.time()
    ref, st, rc = Oracle(sd, cd).render(seed=4)
    print("C4 posed, offset %g: oracle %.1f s, status %d" % (offset, time.time() - t0, rc))
    assert rc == 0
    r = Renderer(sd, cd, device=0)
    mode = r.get_option("sph_mode_effective")
    print("C4 posed, offset %g: sph_mode_effective %d%s"
          % (offset, mode, "" if mode == 6 else " (the 16-bit leaf grid was refused: float32 leaves from global memory)"))
    if offset == 30.0:
        assert mode == 6
    else:
        assert mode in (4, 6)
    fb = r.render(seed=4)
    _check_against_oracle(fb, ref)
    for key, v in (("bvh", 0), ("sphere_src", 2), ("sphere_src", 4)):
        r.set_option("bvh", 1)
        r.set_option("sphere_src", -1)
        r.set_option(key, v)
        assert _same(r.render(seed=4), fb), (key, v)
    r.close()


@pytest.mark.parametrize("seed,bind", [(1, False), (1, True), (6, False), (6, True)])
def test_posed_first_hit(gpu, tmp_path, seed, bind):
    """rtx_first_hit on a posed scene against test_gpu_first_hit.py's reference: with
    no aperture every id and every double bit for bit, misses hold the scaled
    max_distance exactly; with the seed's own aperture the object id wherever the two
    nearest distances are more than 1e-6 max_distance apart (that file's rule)."""
    import fuzz_scenes
    from test_gpu_first_hit import _assert_equal, _bits, _first_hit, expected
    scale = fuzz_scenes.posed_parameters(seed)[0]
    w, c = fuzz_scenes.make_posed(seed, tmp_path, 48, 27, bind_distance=bind)
    exp = expected(w, c, aperture_radius=0.0)
    assert exp["max_distance"] == (9.0 if bind else 10000.0) * scale
    got = _first_hit(w, c, aperture_radius=0.0)
    _assert_equal(got, exp)
    miss = exp["ids"][..., 0] < 0
    print("posed seed %d, bind %d: %d of %d pixels miss" % (seed, bind, miss.sum(), miss.size))
    assert miss.any() and not miss.all()
    rec = np.zeros(10)
    rec[0] = exp["max_distance"]
    assert (got[0][miss] == -1).all() and (_bits(got[1][miss]) == _bits(rec)).all()
    for opts in ((("bvh", 0),), (("bvh", 2),)):
        _assert_equal(_first_hit(w, c, options=opts, aperture_radius=0.0), exp)
    # the seed's own camera (an aperture draws cos / sin: ulps may differ from glibc's)
    exp = expected(w, c, margins=True)
    ids, _ = _first_hit(w, c)
    clear = exp["margin"] > 1e-6 * exp["max_distance"]
    excluded = int((~clear).sum())
    print("posed seed %d, bind %d: %d of %d pixels excluded (two nearest distances within 1e-6 max_distance)"
          % (seed, bind, excluded, clear.size))
    assert excluded <= 0.05 * clear.size, excluded
    assert np.array_equal(ids[..., 0][clear], exp["ids"][..., 0][clear])


def test_posed_render_at_and_subregion(gpu, tmp_path):
    import fuzz_scenes
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    seed = fuzz_scenes.POSED_SEEDS[7]                 # scale 1, offset 1e5, max_distance binds
    w, c = fuzz_scenes.make_posed(seed, tmp_path, 48, 27)
    sd, cd = config.load_scene(w, c)
    r = Renderer(sd, cd, device=0)
    full = r.render(seed=seed)
    assert len(np.unique(full.reshape(-1, 3), axis=0)) > 100
    assert _same(r.render(5, 3, 42, 26, seed=seed), full[3:26, 5:42])
    assert _same(r.render(47, 26, 48, 27, seed=seed), full[26:, 47:])
    for x, y in ((0, 0), (47, 26), (13, 20), (30, 7), (24, 13)):
        assert _same(r.render_at(x, y, seed=seed), full[y, x]), (x, y)
    r.close()
