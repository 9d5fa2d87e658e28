"""First-hit feature buffers (rtx_first_hit, rtx_aov.hip): object id, direction,
box face, depth, position, normal and albedo of one camera sample's primary ray
per pixel -- Camera#lens_func (camera.rb:129-151) -> World#intersect
(world.rb:37-59), no shading.

Expected values come from ``expected()`` below, which walks the Python
restatement of the reference (oracle/rt_ref.py): ``lens_func``,
``world.intersect``, ``intersect_parameters(...)[0].normalize()``, ``get_uv``,
``texture.color``, ``diffuse_rate``.  With ``aperture_radius: 0`` the path needs
no libm function (only + - * / sqrt, trunc, fmod), so doubles are compared on
their uint64 view: there is no tolerance in this file.
"""

import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

IN, OUT = 0, 1


def _paths(name):
    return os.path.join(SCENES, "%s_world.yml" % name), os.path.join(SCENES, "%s_camera.yml" % name)


# ------------------------------------------------------------------ the CPU helper
def _normal_only(obj, ray, intersection, direction, data):
    """intersect_parameters' n alone (sphere.rb:89, plane.rb:55, box.rb:100-105),
    for a hit whose reflection / refraction arithmetic raises after it."""
    from oracle import rt_ref
    if isinstance(obj, rt_ref.Box):
        obj = obj.planes[data]
    if isinstance(obj, rt_ref.Sphere):
        return (intersection - obj.center) if direction == "in" else (obj.center - intersection)
    return -obj.front if obj.front.dot(ray.front) > 0 else obj.front


@functools.lru_cache(maxsize=None)
def _expected(world_yml, camera_yml, sample, margins, ov):
    from oracle import rt_ref
    from oracle.rb_vec3 import RtxError
    world, cam = rt_ref.load_scene(world_yml, camera_yml, seed=1, overrides=dict(ov))
    index = {id(o): i for i, o in enumerate(world.objects)}
    W, H = cam.width, cam.height
    ids = np.full((H, W, 3), -1, np.int32)
    geom = np.zeros((H, W, 10), np.float64)
    margin = np.full((H, W), np.inf)
    for y in range(H):
        for x in range(W):
            ray = cam.lens_func(x, y, sample)
            obj, inter, direction, delta, data = world.intersect(ray)
            if margins:                       # nearest and second-nearest distance World#intersect compares
                ds = [world.max_distance]
                for o in world.objects:
                    res = o.intersect(ray)
                    if res and res[0] is not None:
                        ds.append(ray.distance(res[0]))
                ds.sort()
                margin[y, x] = ds[1] - ds[0] if len(ds) > 1 else np.inf
            if obj is None:
                geom[y, x, 0] = world.max_distance
                continue
            ids[y, x] = (index[id(obj)], IN if direction == "in" else OUT, -1 if data is None else data)
            try:
                n = obj.intersect_parameters(ray, inter, direction, delta, data)[0]
            except RtxError:
                n = _normal_only(obj, ray, inter, direction, data)
            try:
                n = n.normalize().to_a()
            except RtxError:                  # a zero n gives zeros
                n = [0.0, 0.0, 0.0]
            a = obj.diffuse_rate
            if obj.texture is not None and not isinstance(obj, rt_ref.Box):
                try:
                    a = a * obj.texture.color(*obj.get_uv(inter))
                except RtxError:              # a non-finite uv gives zeros
                    a = rt_ref.Vec3(0.0, 0.0, 0.0)
            geom[y, x] = [ray.distance(inter)] + inter.to_a() + n + a.to_a()
    kinds = [type(o).__name__ for o in world.objects]
    textured = [o.texture is not None and not isinstance(o, rt_ref.Box) for o in world.objects]
    for a in (ids, geom, margin):
        a.setflags(write=False)               # shared among the tests: left unchanged
    return {"ids": ids, "geom": geom, "margin": margin, "kinds": kinds, "textured": textured,
            "max_distance": float(world.max_distance)}


def expected(world_yml, camera_yml, sample=0, margins=False, **ov):
    return _expected(world_yml, camera_yml, sample, margins, tuple(sorted(ov.items())))


# ------------------------------------------------------------------ GPU side
def _renderer(world_yml, camera_yml, **ov):
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    sd, cd = config.load_scene(world_yml, camera_yml, camera_overrides=ov)
    return Renderer(sd, cd, device=0)


def _buffers(g):
    """(ids [H, W, 3], geom [H, W, 10]) of a first_hit dict."""
    ids = np.stack([g["object"], g["direction"], g["data"]], axis=-1)
    geom = np.concatenate([g["depth"][..., None], g["position"], g["normal"], g["albedo"]], axis=-1)
    return np.ascontiguousarray(ids), np.ascontiguousarray(geom)


def _first_hit(world_yml, camera_yml, sample=0, options=(), rect=(), **ov):
    r = _renderer(world_yml, camera_yml, **ov)
    for k, v in options:
        r.set_option(k, v)
    g = r.first_hit(*rect, sample=sample)
    r.close()
    return _buffers(g)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_equal(got, exp):
    ids, geom = got
    assert ids.dtype == np.int32 and geom.dtype == np.float64
    assert ids.shape == exp["ids"].shape and geom.shape == exp["geom"].shape
    bad = np.argwhere((ids != exp["ids"]).any(axis=-1))
    assert len(bad) == 0, ("ids differ at (row, col)", bad[:5].tolist(), ids[tuple(bad[0])], exp["ids"][tuple(bad[0])])
    bad = np.argwhere((_bits(geom) != _bits(exp["geom"])).any(axis=-1))
    assert len(bad) == 0, ("geom bits differ at (row, col)", bad[:5].tolist(), geom[tuple(bad[0])].tolist(),
                           exp["geom"][tuple(bad[0])].tolist())


def _check_misses(got, exp):
    ids, geom = got
    miss = exp["ids"][..., 0] < 0
    assert miss.any(), "the frame has no miss"
    assert (ids[miss] == -1).all()
    rec = np.zeros(10)
    rec[0] = exp["max_distance"]
    assert (_bits(geom[miss]) == _bits(rec)).all()


@pytest.fixture(scope="module")
def c4_world():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_scenes
    return make_scenes.ensure_c4()


MIX = dict(width=48, height=27, aperture_radius=0.0)


# 1 ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_mix_equals_reference(gpu):
    """Textured plane, box, textured sphere, glass sphere, two more planes."""
    w, c = _paths("mix")
    exp = expected(w, c, **MIX)
    seen = set(int(k) for k in np.unique(exp["ids"][..., 0]) if k >= 0)
    kinds = {exp["kinds"][k] for k in seen}
    assert {"Sphere", "Plane", "Box"} <= kinds, kinds
    box = exp["ids"][..., 0] == exp["kinds"].index("Box")
    assert box.any() and (exp["ids"][box][:, 2] >= 0).all() and (exp["ids"][~box][:, 2] == -1).all()
    assert any(exp["textured"][k] for k in seen)
    _assert_equal(_first_hit(w, c, **MIX), exp)


# 2 ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,ov", [("c2", dict(width=32, height=18)), ("c1", dict(width=24, height=14))])
def test_sphere_scenes_equal_reference_with_misses(gpu, name, ov):
    w, c = _paths(name)
    exp = expected(w, c, aperture_radius=0.0, **ov)
    got = _first_hit(w, c, aperture_radius=0.0, **ov)
    _assert_equal(got, exp)
    _check_misses(got, exp)


# 3 ---------------------------------------------------------------------------
_OUT_WORLD = """max_distance: 10000
soft_shadow_exponent: 2
lights:
  - type: Spot
    properties:
      name: Main
      position: [1.0, -1.0, 2.0]
      radius: 0.5
      color: [1.0, 1.0, 1.0]
      high_light_rate: 1.0
      high_light_angle: 3.0
world_objects:
  - type: Sphere
    properties:
      name: shell
      center: [0.0, 0.0, 0.0]
      radius: 5.0
      refractive_rate: 1.5
      diffuse_rate: [0.1, 0.2, 0.3]
      ambient: [0.01, 0.01, 0.01]
      reflective_attenuation: [0.1, 0.1, 0.1]
      refractive_attenuation: [0.8, 0.8, 0.8]
  - type: Plane
    properties:
      name: seen from behind
      point: [4.0, 0.0, 0.0]
      front: [1.0, 1.0, 0.0]
      up: [0.0, 0.0, 1.0]
      diffuse_rate: [0.6, 0.5, 0.4]
      reflective_attenuation: [0.3, 0.3, 0.3]
      ambient: [0.05, 0.05, 0.05]
  - type: Box
    properties:
      name: crate
      point: [3.0, -1.0, -0.6]
      front: [1.0, 0.3, 0.0]
      up: [0.0, 0.0, 1.0]
      width_front: 0.8
      width_up: 0.9
      width_left: 0.7
      refractive_rate: 1.3
      diffuse_rate: [0.3, 0.25, 0.2]
      ambient: [0.02, 0.02, 0.02]
      reflective_attenuation: [0.2, 0.2, 0.2]
      refractive_attenuation: [0.3, 0.3, 0.3]
"""


def _out_scene(tmp_path):
    p = tmp_path / "out_world.yml"
    p.write_text(_OUT_WORLD)
    return str(p), os.path.join(SCENES, "mix_camera.yml")


@pytest.mark.gpu
def test_out_hits(gpu, tmp_path):
    """The camera inside a large refractive sphere (every sphere hit is :out), a
    plane whose front points away from the camera (front.dot(ray.front) > 0:
    :out, plane.rb:45-49) cutting the view, and a box."""
    w, c = _out_scene(tmp_path)
    ov = dict(width=16, height=9, aperture_radius=0.0)
    exp = expected(w, c, **ov)
    obj, direction = exp["ids"][..., 0], exp["ids"][..., 1]
    assert (direction[obj == 0] == OUT).any() and (direction[obj == 1] == OUT).any()
    assert (obj == 2).any()
    _assert_equal(_first_hit(w, c, **ov), exp)


# 4 ---------------------------------------------------------------------------
def _walks_agree(r):
    """The ordered linear walk ("bvh" 0) and the hierarchy ("bvh" 2) of one renderer."""
    for sample in (0, 1):
        r.set_option("bvh", 0)
        lin = _buffers(r.first_hit(sample=sample))
        r.set_option("bvh", 2)
        bvh = _buffers(r.first_hit(sample=sample))
        r.set_option("sphere_src", 1)                             # the hierarchy read from global memory
        glb = _buffers(r.first_hit(sample=sample))
        r.set_option("sphere_src", -1)
        for got in (bvh, glb):
            assert np.array_equal(lin[0], got[0]), sample
            assert np.array_equal(_bits(lin[1]), _bits(got[1])), sample
        assert (lin[0][..., 0] >= 0).any()
    r.set_option("bvh", 1)                                        # the default again


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2", "mix"])
def test_hierarchy_and_linear_walk_agree(gpu, name):
    r = _renderer(*_paths(name), width=96, height=54)
    _walks_agree(r)
    r.close()


@pytest.fixture(scope="module")
def c4_renderer(gpu, c4_world):
    """One upload of the 4,096 spheres for both C4 tests (each sets its camera)."""
    r = _renderer(c4_world, os.path.join(SCENES, "c4_camera.yml"), width=16, height=9)
    yield r
    r.close()


def _c4_camera(r, **ov):
    from raytracing_rb_amd import config
    r.set_camera(config.build_camera(dict(config.load_yaml(os.path.join(SCENES, "c4_camera.yml")), **ov)))


@pytest.mark.gpu
def test_c4_hierarchy_and_linear_walk_agree(gpu, c4_renderer):
    """4,096 spheres: by default the hierarchy is read from global memory (its 101 KB
    of records in LDS would leave one workgroup per CU); C2 and mix stage theirs."""
    _c4_camera(c4_renderer, width=256, height=144)
    _walks_agree(c4_renderer)


@pytest.mark.gpu
def test_c4_default_options_equal_reference(gpu, c4_world, c4_renderer):
    ov = dict(width=16, height=9, aperture_radius=0.0)
    exp = expected(c4_world, os.path.join(SCENES, "c4_camera.yml"), **ov)
    assert (exp["ids"][..., 0] >= 0).any()
    _c4_camera(c4_renderer, **ov)
    assert c4_renderer.get_option("bvh") == 1 and c4_renderer.get_option("sphere_src") == -1
    _assert_equal(_buffers(c4_renderer.first_hit()), exp)


# 5 ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_rectangles_and_edges(gpu):
    import torch
    w, c = _paths("mix")
    exp = expected(w, c, **MIX)
    r = _renderer(w, c, **MIX)
    ids, geom = _buffers(r.first_hit(5, 3, 42, 26))
    assert np.array_equal(ids, exp["ids"][3:26, 5:42])
    assert np.array_equal(_bits(geom), _bits(exp["geom"][3:26, 5:42]))
    ids, geom = _buffers(r.first_hit(47, 26, 48, 27))            # 1 x 1 at the last pixel
    assert ids.shape == (1, 1, 3) and np.array_equal(ids, exp["ids"][26:, 47:])
    assert np.array_equal(_bits(geom), _bits(exp["geom"][26:, 47:]))
    # one buffer at a time: the other (poisoned) is untouched
    d_ids = torch.full((27, 48, 3), -77, dtype=torch.int32, device=gpu)
    d_geom = torch.full((27, 48, 10), -77.0, dtype=torch.float64, device=gpu)
    r.first_hit_device(None, d_geom.data_ptr())
    torch.cuda.synchronize()
    assert bool((d_ids == -77).all())
    assert np.array_equal(_bits(d_geom.cpu().numpy()), _bits(exp["geom"]))
    d_geom.fill_(-77.0)
    r.first_hit_device(d_ids.data_ptr(), None)
    torch.cuda.synchronize()
    assert bool((d_geom == -77.0).all())
    assert np.array_equal(d_ids.cpu().numpy(), exp["ids"])
    r.close()
    # smaller than two tiles, no multiple of 8
    ov = dict(width=13, height=7, aperture_radius=0.0)
    _assert_equal(_first_hit(w, c, **ov), expected(w, c, **ov))


# 6 ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_samples(gpu):
    w, c = _paths("mix")
    r = _renderer(w, c, **MIX)
    n = r.camera.max_sample_times
    assert n == 6
    first = _buffers(r.first_hit(sample=0))
    for j in range(1, n):                                         # no aperture: the sample changes nothing
        got = _buffers(r.first_hit(sample=j))
        assert np.array_equal(got[0], first[0]) and np.array_equal(_bits(got[1]), _bits(first[1])), j
    r.close()
    # the camera's own aperture: the lens ray's cos / sin may differ from glibc's by
    # ulps, so only pixels with a clear winner are compared, and only the object
    ov = dict(width=24, height=14)
    r = _renderer(w, c, **ov)
    got = [r.first_hit(sample=j) for j in (0, 1)]
    r.close()
    assert (_bits(got[0]["position"]) != _bits(got[1]["position"])).any()
    for j in (0, 1):
        exp = expected(w, c, sample=j, margins=True, **ov)
        clear = exp["margin"] > 1e-6 * exp["max_distance"]
        excluded = int((~clear).sum())
        print("sample %d: %d of %d pixels excluded (two nearest distances within 1e-6 max_distance)"
              % (j, excluded, clear.size))
        assert excluded <= 0.05 * clear.size, excluded
        assert np.array_equal(got[j]["object"][clear], exp["ids"][..., 0][clear]), j


# 7 ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_and_raise_state(gpu, tmp_path):
    from raytracing_rb_amd.runtime import RtxError
    w, c = _paths("c1")
    ov = dict(width=24, height=14)
    r = _renderer(w, c, **ov)
    n = max(r.camera.pre_sample_times, r.camera.max_sample_times)
    ids = np.zeros((14, 24, 3), np.int32)
    geom = np.zeros((14, 24, 10))
    pi, pg = ids.ctypes.data_as(C.POINTER(C.c_int32)), geom.ctypes.data_as(C.POINTER(C.c_double))
    for bad in ((0, 0, 24, 14, 1, n, pi, pg), (0, 0, 24, 14, 1, -1, pi, pg),       # sample
                (5, 3, 5, 9, 1, 0, pi, pg), (5, 9, 8, 3, 1, 0, pi, pg),              # empty
                (0, 0, 25, 14, 1, 0, pi, pg), (0, 0, 24, 15, 1, 0, pi, pg), (-1, 0, 24, 14, 1, 0, pi, pg),
                (0, 0, 24, 14, 1, 0, None, None)):                                    # both NULL
        assert r.lib.rtx_first_hit(r.h, *bad) == 6, bad[:6]                          # RTX_EINVAL
    assert r.lib.rtx_first_hit_device(r.h, 0, 0, 24, 14, 1, 0, None, None, None) == 6
    with pytest.raises(RtxError) as e:
        r.first_hit(sample=n)
    assert e.value.kind == "invalid"
    before = r.render()
    g = r.first_hit()
    assert (g["object"] >= 0).any()
    assert np.array_equal(_bits(r.render()), _bits(before))
    r.close()
    # a scene whose colour path raises ("color greater than 1"): the pass records nothing
    src = open(w).read()
    src = src.replace("diffuse_rate:           [0.5, 0.5, 0.5]", "diffuse_rate:           [0.99, 0.99, 0.99]")
    src = src.replace("ambient:                [0.05, 0.05, 0.05]", "ambient:                [0.3, 0.3, 0.3]", 1)
    p = tmp_path / "bright.yml"
    p.write_text(src)
    r = _renderer(str(p), c, **ov)
    with pytest.raises(RtxError) as e:
        r.render()
    assert e.value.kind == "color_gt1"
    r.first_hit()
    r.sync()                                                      # RTX_OK: raises nothing
    r.close()


# 8 ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_api_shapes(gpu):
    from raytracing_rb_amd.api import Camera, World
    w, c = _paths("mix")
    cam = Camera(World(w), c, width=40, height=23)
    g = cam.first_hit()
    assert sorted(g) == ["albedo", "data", "depth", "direction", "normal", "object", "position"]
    for k in ("object", "direction", "data"):
        assert g[k].shape == (23, 40) and g[k].dtype == np.int32, k
    assert g["depth"].shape == (23, 40) and g["depth"].dtype == np.float64
    for k in ("position", "normal", "albedo"):
        assert g[k].shape == (23, 40, 3) and g[k].dtype == np.float64, k
    assert cam.first_hit(sample=1, x0=8, y0=4, x1=19, y1=9)["depth"].shape == (5, 11)
    hit = g["object"] >= 0
    assert hit.any() and np.allclose(np.linalg.norm(g["normal"][hit], axis=-1), 1.0, atol=1e-12)


@pytest.mark.gpu
def test_cli_geometry_mode(gpu, tmp_path):
    """`rtx g` and `python -m raytracing_rb_amd g`: three PNGs of the frame's size,
    the normal picture = trunc(min(256 (n + 1) / 2, 255)) under the png gem's blend
    over black ((b * 255) >> 8), as a colour frame is written."""
    from raytracing_rb_amd import _build, png
    from raytracing_rb_amd.__main__ import main
    from raytracing_rb_amd.api import Camera, World
    w, c = _paths("mix")
    cli = _build.build_cli()
    out = str(tmp_path / "geo.png")
    r = subprocess.run([cli, "g", out, w, c], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert main(["g", str(tmp_path / "py.png"), w, c]) == 0
    cam = Camera(World(w), c)
    g = cam.first_hit()
    H, W = cam.height, cam.width
    for name in ("normal", "depth", "albedo"):
        p = str(tmp_path / ("geo.%s.png" % name))
        assert png.decode_rgb8(p).shape == (H, W, 3), name
        assert open(p, "rb").read() == open(tmp_path / ("py.%s.png" % name), "rb").read(), name
    b = np.trunc(np.minimum(256.0 * ((g["normal"] + 1.0) / 2.0), 255.0)).astype(np.int64)
    assert np.array_equal(png.decode_rgb8(str(tmp_path / "geo.normal.png")), (b * 255) >> 8)
    assert not os.path.exists(out)


# CPU ---------------------------------------------------------------------------
def test_symbols_and_bindings():
    """Both entry points are exported by the built library with the signatures
    _abi.py declares, and the Ruby binding names them."""
    from raytracing_rb_amd import _abi
    lib = _abi.load_library()
    sig = {name: (res, args) for name, res, args in _abi.SIGNATURES}
    I, P, U64 = C.c_int32, C.c_void_p, C.c_uint64
    assert sig["rtx_first_hit_device"] == (I, [P, I, I, I, I, U64, I, P, P, P])
    assert sig["rtx_first_hit"] == (I, [P, I, I, I, I, U64, I, C.POINTER(C.c_int32), C.POINTER(C.c_double)])
    for name in ("rtx_first_hit_device", "rtx_first_hit"):
        fn = getattr(lib, name)
        assert fn.restype is sig[name][0] and list(fn.argtypes) == sig[name][1]
    assert lib.rtx_first_hit(None, 0, 0, 1, 1, 1, 0, None, None) == 6      # RTX_EINVAL: no context
    rb = open(os.path.join(ROOT, "ext", "rtx", "lib", "rtx.rb")).read()
    assert "extern 'int rtx_first_hit_device(" in rb and "extern 'int rtx_first_hit(" in rb
