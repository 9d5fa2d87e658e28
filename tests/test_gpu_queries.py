"""Batched World queries (rtx_intersect, rtx_lit_area; rtx_aov.hip k_intersect,
rtx_query.hip k_lit_area): World#intersect (world.rb:37-59), World#lit_area
(world.rb:62-69) and World#local_lights (world.rb:72-80) for explicit rays and
targets.

Expected values come from the Python restatement of the reference
(oracle/rt_ref.py): ``world.intersect``, ``world.lit_area``,
``world.local_lights``, with the normal and the albedo taken as
tests/test_gpu_first_hit.py's ``_expected`` takes them.  Doubles are compared on
their uint64 view.  The one tolerance: a (target, light) pair whose lit_area calls
Math.acos (a partial cover) is compared within 1e-9, the project's max-|diff|
bound, because libm's acos / sin and the device's differ
in the last bits; a pair that calls none is compared bit for bit.
"""

import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-9                    # DESIGN.md section 6 (max |diff|); only where the oracle calls acos
EINVAL, EDOMAIN = 6, 3
NAMES = ("rtx_intersect_device", "rtx_intersect", "rtx_lit_area_device", "rtx_lit_area")


def _paths(name):
    return os.path.join(SCENES, "%s_world.yml" % name), os.path.join(SCENES, "%s_camera.yml" % name)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _renderer(world_yml, camera_yml, options=(), **ov):
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    sd, cd = config.load_scene(world_yml, camera_yml, camera_overrides=ov)
    r = Renderer(sd, cd, device=0)
    for k, v in options:
        r.set_option(k, v)
    return r


def _buffers(g):
    """(ids [n, 3], geom [n, 13]) of an intersect dict."""
    ids = np.stack([g["object"], g["direction"], g["data"]], axis=-1)
    geom = np.concatenate([g["depth"][..., None], g["position"], g["normal"], g["albedo"], g["delta"]], axis=-1)
    return np.ascontiguousarray(ids), np.ascontiguousarray(geom)


# ------------------------------------------------------------------ the CPU side
@functools.lru_cache(maxsize=None)
def _oracle_world(world_yml, camera_yml):
    from oracle import rt_ref
    return rt_ref.load_scene(world_yml, camera_yml)[0]


def _oracle_ray(row):
    from oracle import rt_ref
    from oracle.rb_vec3 import Vec3
    v = [float(x) for x in row]            # Python floats: Plane#intersect fails on numpy booleans
    return rt_ref.Ray(Vec3(*v[:3]), Vec3(*v[3:]))


def expected_intersect(world, rays):
    """ids [n, 3], geom [n, 13] of world.intersect, and per ray the indices of the
    objects at the nearest distance (more than one: a tie)."""
    from oracle import rt_ref
    from oracle.rb_vec3 import RtxError
    from test_gpu_first_hit import _normal_only
    index = {id(o): i for i, o in enumerate(world.objects)}
    n = len(rays)
    ids = np.full((n, 3), -1, np.int32)
    geom = np.zeros((n, 13), np.float64)
    nearest = []
    for i in range(n):
        ray = _oracle_ray(rays[i])
        obj, inter, direction, delta, data = world.intersect(ray)
        ds = []
        for k, o in enumerate(world.objects):
            res = o.intersect(ray)
            if res and res[0] is not None:
                ds.append((ray.distance(res[0]), k))
        dmin = min(d for d, _ in ds) if ds else None
        nearest.append([k for d, k in ds if d == dmin and d < world.max_distance])
        if obj is None:
            geom[i, 0] = world.max_distance
            continue
        ids[i] = (index[id(obj)], 0 if direction == "in" else 1, -1 if data is None else data)
        try:
            nv = obj.intersect_parameters(ray, inter, direction, delta, data)[0]
        except RtxError:
            nv = _normal_only(obj, ray, inter, direction, data)
        try:
            nv = nv.normalize().to_a()
        except RtxError:                      # a zero n gives zeros
            nv = [0.0, 0.0, 0.0]
        a = obj.diffuse_rate
        if obj.texture is not None and not isinstance(obj, rt_ref.Box):
            try:
                a = a * obj.texture.color(*obj.get_uv(inter))
            except RtxError:                  # a non-finite uv gives zeros
                a = rt_ref.Vec3(0.0, 0.0, 0.0)
        geom[i] = [ray.distance(inter)] + inter.to_a() + nv + a.to_a() + delta.to_a()
    return ids, geom, nearest


class _AcosCount:
    """Counts rt_ref._acos calls (the only libm function of World#lit_area besides sin, which follows it)."""

    def __enter__(self):
        from oracle import rt_ref
        self.mod, self.orig, self.n = rt_ref, rt_ref._acos, 0

        def counted(x):
            self.n += 1
            return self.orig(x)
        rt_ref._acos = counted
        return self

    def __exit__(self, *exc):
        self.mod._acos = self.orig


def expected_lit_area(world, targets, lights=None):
    """area [n, L], color [n, L, 3], acos calls [n, L], raised [n] (bool; entries from the raise on: NaN).
    lights None: the world's lights (local_lights); else one explicit (x, y, z, radius) per target."""
    from oracle.rb_vec3 import RtxError, Vec3
    n = len(targets)
    L = 1 if lights is not None else len(world.lights)
    area = np.full((n, L), np.nan)
    color = np.full((n, L, 3), np.nan)
    calls = np.zeros((n, L), np.int64)
    raised = np.zeros(n, bool)
    for i in range(n):
        T = Vec3(*[float(v) for v in targets[i]])
        for k in range(L):
            if lights is not None:
                pos, rad, col = Vec3(*[float(v) for v in lights[i][:3]]), float(lights[i][3]), None
            else:
                pos, rad, col = world.lights[k].position, world.lights[k].radius, world.lights[k].color
            with _AcosCount() as cnt:
                try:
                    a = float(world.lit_area(T, pos, rad))
                except RtxError:
                    raised[i] = True
            calls[i, k] = cnt.n
            if raised[i]:
                break
            area[i, k] = a
            if col is not None:               # world.rb:76-77
                color[i, k] = (col * (a ** world.soft_shadow_exponent / len(world.lights))).to_a() if a > 0 else 0.0
    return area, color, calls, raised


def assert_lit_area(got_area, got_color, exp, where=""):
    """Case 3's rule: bit for bit where the oracle calls no acos, else within TOL; the colour
    within TOL everywhere and exactly zero where the oracle's area is 0."""
    area, color, calls, raised = exp
    ok = ~np.isnan(area)
    free = ok & (calls == 0)
    diff = np.abs(np.where(ok, got_area - area, 0.0))
    print("%s: %d entries, %d libm-free, max |diff| %.3e" % (where, ok.sum(), free.sum(), diff.max() if ok.any() else 0))
    bad = np.argwhere(free & (_bits(got_area) != _bits(area)))
    assert len(bad) == 0, (where, "libm-free areas differ", bad[:5].tolist(),
                           got_area[tuple(bad[0])], area[tuple(bad[0])])
    assert (diff <= TOL).all(), (where, float(diff.max()))
    assert np.isnan(got_area[~ok]).all(), where
    if got_color is not None:
        okc = ~np.isnan(color)
        assert (np.abs(np.where(okc, got_color - color, 0.0)) <= TOL).all(), where
        assert (got_color[ok & (area == 0)] == 0).all(), where
        assert np.isnan(got_color[~okc]).all(), where


@functools.lru_cache(maxsize=None)
def _table(name):
    """Case 1's expected values of test_gpu_rays.ray_table(name), computed once."""
    from test_gpu_rays import ray_table
    labels, rays, keys, far = ray_table(name)
    world = _oracle_world(*_paths(name))
    ids, geom, nearest = expected_intersect(world, rays)
    for a in (ids, geom):
        a.setflags(write=False)
    return rays, ids, geom, nearest


@functools.lru_cache(maxsize=None)
def _table_targets(name):
    """Case 3: the targets intersection + delta of the table's hits and their expected lit areas."""
    from oracle.rb_vec3 import Vec3
    rays, ids, geom, _ = _table(name)
    hit = ids[:, 0] >= 0
    T = np.array([(Vec3(*g[1:4].tolist()) + Vec3(*g[10:13].tolist())).to_a() for g in geom[hit]], np.float64)
    exp = expected_lit_area(_oracle_world(*_paths(name)), T)
    for a in (T,) + exp:
        a.setflags(write=False)
    return T, exp


# 1 ---------------------------------------------------------------------------
TABLE_COUNTS = {"mix": (85, 72, 13, 1), "c2": (171, 146, 25, 3)}      # rays, hits, misses, ties


@pytest.mark.parametrize("name", ("mix", "c2"))
def test_table_conditions(name):
    """By the oracle alone: the table's hits, misses and ties, and case 3's populations."""
    rays, ids, geom, nearest = _table(name)
    ties = [i for i, ks in enumerate(nearest) if len(ks) > 1]
    hits = int((ids[:, 0] >= 0).sum())
    print(name, len(rays), hits, len(rays) - hits, len(ties))
    assert (len(rays), hits, len(rays) - hits, len(ties)) == TABLE_COUNTS[name]
    for i in ties:                               # the lower YAML index wins (strict <, world.rb:44)
        assert ids[i, 0] == min(nearest[i]), (i, nearest[i], ids[i])
    T, (area, color, calls, raised) = _table_targets(name)
    assert not raised.any()
    partial = (area > 0) & (area < 1)
    print(name, area.size, int((area == 0).sum()), int((area == 1).sum()), int(partial.sum()), int((calls == 0).sum()))
    assert partial.any() and (area == 0).any() and (area == 1).any()
    assert (calls == 0).sum() * 2 >= calls.size


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("mix", "c2"))
def test_intersect_degenerate_rays(gpu, name):
    """All 13 + 3 values of every ray of the degenerate-ray tables, misses included, bit for bit."""
    rays, ids, geom, nearest = _table(name)
    r = _renderer(*_paths(name), width=40, height=24)
    got_ids, got_geom = _buffers(r.intersect(rays))
    r.close()
    assert got_ids.dtype == np.int32 and got_ids.shape == ids.shape and got_geom.shape == geom.shape
    bad = np.nonzero((got_ids != ids).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5].tolist(), got_ids[bad[0]], ids[bad[0]])
    bad = np.nonzero((_bits(got_geom) != _bits(geom)).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5].tolist(), got_geom[bad[0]].tolist(), geom[bad[0]].tolist())
    ties = [i for i, ks in enumerate(nearest) if len(ks) > 1]
    assert ties
    for i in ties:
        assert got_ids[i, 0] == min(nearest[i])
    miss = ids[:, 0] < 0
    rec = np.zeros(13)
    rec[0] = _oracle_world(*_paths(name)).max_distance
    assert miss.any() and (got_ids[miss] == -1).all() and (_bits(got_geom[miss]) == _bits(rec)).all()


# 2 ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_intersect_equals_first_hit(gpu):
    """The oracle's lens rays of mix at 48 x 27, aperture 0, through rtx_intersect: ids and the
    first ten geom columns are rtx_first_hit's of the same renderer."""
    from oracle import rt_ref
    ov = dict(width=48, height=27, aperture_radius=0.0)
    w, c = _paths("mix")
    _, cam = rt_ref.load_scene(w, c, overrides=dict(ov))
    rays = np.array([(lambda ray: ray.front.to_a() + ray.position.to_a())(cam.lens_func(x, y, 0))
                     for y in range(27) for x in range(48)], np.float64)
    r = _renderer(w, c, **ov)
    fh = r.first_hit()
    got_ids, got_geom = _buffers(r.intersect(rays))
    r.close()
    fh_ids = np.stack([fh["object"], fh["direction"], fh["data"]], axis=-1).reshape(-1, 3)
    fh_geom = np.concatenate([fh["depth"][..., None], fh["position"], fh["normal"], fh["albedo"]], axis=-1).reshape(-1, 10)
    assert len(np.unique(fh_ids[:, 0])) >= 3                     # (several objects in the frame)
    assert np.array_equal(got_ids, fh_ids)
    assert np.array_equal(_bits(got_geom[:, :10]), _bits(fh_geom))


# 3 ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("mix", "c2"))
def test_lit_area_at_table_targets(gpu, name):
    T, exp = _table_targets(name)
    r = _renderer(*_paths(name), width=40, height=24)
    area, color, status = r.lit_area(T)
    r.close()
    assert area.shape == exp[0].shape and color.shape == exp[1].shape
    assert (status == 0).all()
    assert_lit_area(area, color, exp, name)


# 4 ---------------------------------------------------------------------------
def _six_cover_world(tmp_path, fillers):
    import test_raises as tr
    src = "max_distance: 10000\nsoft_shadow_exponent: 2\n" + tr._light((0.0, 0.0, 10.0), 2.0, 1.0) + "world_objects:\n"
    for k in range(6):
        z = 1.0 + k
        R = 0.06 * z
        src += tr._sphere("s%d" % k, (0.5 * R * np.cos(k), 0.5 * R * np.sin(k), z), R)
    src += tr._fillers(fillers)
    w = tmp_path / ("six_%d.yml" % fillers)
    w.write_text(src)
    return str(w), tr._camera(tmp_path, (0.0, -8.0, 2.0), (0.0, 1.0, -0.2))


SIX = 0.4600000000000002


def test_six_covers_oracle(tmp_path):
    from oracle import rt_ref
    from oracle.rb_vec3 import Vec3
    for fillers in (0, 40):
        world = rt_ref.load_scene(*_six_cover_world(tmp_path, fillers))[0]
        T, L = Vec3(0.0, 0.0, 0.0), Vec3(0.0, 0.0, 10.0)
        with _AcosCount() as cnt:
            covers = [o.cover_area(L, 2.0, T) for o in world.objects]
            assert world.lit_area(T, L, 2.0) == SIX
        assert cnt.n == 0
        nz = [c for c in covers if c != 0]
        assert len(nz) == 6 and set(nz) <= {0.09, 0.08999999999999998}, nz


@pytest.mark.gpu
@pytest.mark.parametrize("fillers,options", [(0, (("bvh", 0),)), (0, (("bvh", 2),)),
                                             (0, (("bvh", 2), ("sphere_src", 1))), (40, ())])
def test_more_covers_than_the_list_holds(gpu, tmp_path, fillers, options):
    """Six non-zero covers against COVER_K = 4: the ordered sum decides the last bits."""
    r = _renderer(*_six_cover_world(tmp_path, fillers), options=options)
    a_scene, color, st_scene = r.lit_area([[0.0, 0.0, 0.0]])
    a_expl, _, st_expl = r.lit_area([[0.0, 0.0, 0.0]], lights=[[0.0, 0.0, 10.0, 2.0]])
    r.close()
    assert st_scene[0] == 0 and st_expl[0] == 0
    assert a_scene.shape == (1, 1) and a_expl.shape == (1, 1)
    assert _bits(a_scene)[0, 0] == _bits(np.float64(SIX)), a_scene
    assert _bits(a_expl)[0, 0] == _bits(np.float64(SIX)), a_expl
    assert np.abs(color[0, 0] - 0.5 * SIX * SIX).max() <= TOL


# 5 ---------------------------------------------------------------------------
def _raise_batch(world, c):
    """130 targets, the raising T at index 65, the others T displaced by multiples of 1e-3
    along the first axis on which the oracle raises on none of them."""
    T, light = np.array(c["T"], np.float64), list(c["L"]) + [c["light_radius"]]
    for axis in np.eye(3):
        targets = np.array([T + (i - 65) * 1e-3 * axis for i in range(130)])
        lights = np.array([light] * 130, np.float64)
        exp = expected_lit_area(world, targets, lights)
        if exp[3].sum() == 1 and exp[3][65]:
            return targets, lights, exp
    raise AssertionError("every displacement raises somewhere")


@pytest.mark.gpu
@pytest.mark.parametrize("fillers", (0, 40, 300))
@pytest.mark.parametrize("case", ("highlight", "shadow_A", "shadow_B", "pixel_A_back", "pixel_B_front", "pixel_A_far"))
def test_raises(gpu, tmp_path, case, fillers):
    import test_raises as tr
    from oracle import rt_ref
    from raytracing_rb_amd.runtime import RtxError
    c = tr.CASES[case]
    w = tr._world(tmp_path, case, 1.0, fillers=fillers)
    cam = tr._camera(tmp_path, (0.0, -8.0, 2.0), (0.0, 1.0, -0.2))
    targets, lights, exp = _raise_batch(rt_ref.load_scene(w, cam)[0], c)
    r = _renderer(w, cam)

    def render():
        try:
            return 0, r.render()
        except RtxError as e:
            return e.status, None
    before = render()
    area, _, status = r.lit_area(targets, lights=lights, check=False)
    want = np.zeros(130, np.int32)
    want[65] = EDOMAIN
    assert np.array_equal(status, want), np.nonzero(status != want)[0]
    assert_lit_area(area, None, exp, "%s/%d" % (case, fillers))          # (NaN at 65 and there only)
    with pytest.raises(RtxError) as e:                                    # the host call returns 3 and names the index
        r.lit_area(targets, lights=lights)
    assert e.value.status == EDOMAIN and "query 65" in str(e.value), str(e.value)
    # the same sphere with the light as the scene's light (lights == NULL)
    area2, color2, status2 = r.lit_area(targets, check=False)
    assert np.array_equal(status2, want)
    assert np.array_equal(_bits(area2[status2 == 0]), _bits(area[status2 == 0]))
    assert np.isnan(area2[65]).all() and np.isnan(color2[65]).all()
    # nothing went to rtx_sync's state, and the colour path is where it was
    r.sync()
    after = render()
    r.close()
    assert before[0] == after[0]
    if before[1] is not None:
        assert np.array_equal(_bits(before[1]), _bits(after[1]))


# 6, 7 ------------------------------------------------------------------------
WALKS = ((("bvh", 0),), (("bvh", 2),), (("bvh", 2), ("sphere_src", 1)))
N_BATCH = 4097                                  # no multiple of 64 or 256


def _c4_world():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_scenes
    return make_scenes.ensure_c4()


def _random_rays(world_yml, n, seed):
    """Origins inside the box of the scene's sphere centres, directions at random."""
    from raytracing_rb_amd import config
    cfg = config.load_yaml(world_yml)
    cs = np.array([[float(v) for v in o["properties"]["center"]] for o in cfg["world_objects"] if o["type"] == "Sphere"])
    rng = np.random.default_rng(seed)
    o = rng.uniform(cs.min(axis=0), cs.max(axis=0), size=(n, 3))
    d = rng.normal(size=(n, 3))
    return np.ascontiguousarray(np.concatenate([d, o], axis=1))


def _query_all(r, rays):
    ids, geom = _buffers(r.intersect(rays))
    hit = ids[:, 0] >= 0
    T = np.ascontiguousarray(geom[hit, 1:4] + geom[hit, 10:13])
    area, color, status = r.lit_area(T, check=False)
    return ids, geom, T, area, color, status


def _same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def c2_batch(gpu):
    w, c = _paths("c2")
    rays = _random_rays(w, N_BATCH, 11)
    r = _renderer(w, c, width=40, height=24)
    out = _query_all(r, rays)
    for a in (rays,) + out:
        a.setflags(write=False)
    yield r, rays, out
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ("c2", "c4"))
def test_walks_agree(gpu, scene):
    """The ordered walk, the hierarchy and the hierarchy read from global memory: the same bits."""
    w = _paths("c2")[0] if scene == "c2" else _c4_world()
    rays = _random_rays(w, N_BATCH, 11)
    r = _renderer(w, _paths("c2")[1], width=40, height=24)
    got = []
    for opts in WALKS:
        for k, v in opts:
            r.set_option(k, v)
        got.append(_query_all(r, rays))
    r.close()
    ids, geom, T, area, color, status = got[0]
    hits = int((ids[:, 0] >= 0).sum())
    print(scene, "hits", hits, "of", N_BATCH, "shadowed", int((area == 0).sum()), "partial", int(((area > 0) & (area < 1)).sum()))
    assert 0 < hits < N_BATCH and (area == 0).any() and (area > 0).any()
    for other in got[1:]:
        assert _same(got[0], other)


@pytest.mark.gpu
def test_batch_independence(gpu, c2_batch):
    r, rays, full = c2_batch
    ids, geom, T, area, color, status = full
    perm = np.random.default_rng(3).permutation(N_BATCH)
    p_ids, p_geom = _buffers(r.intersect(rays[perm]))
    assert np.array_equal(p_ids, ids[perm]) and np.array_equal(_bits(p_geom), _bits(geom[perm]))
    permT = np.random.default_rng(4).permutation(len(T))
    p_area, p_color, p_status = r.lit_area(T[permT], check=False)
    assert np.array_equal(_bits(p_area), _bits(area[permT])) and np.array_equal(_bits(p_color), _bits(color[permT]))
    assert np.array_equal(p_status, status[permT])
    for n in (1, 63, 64, 65, 257):
        s_ids, s_geom = _buffers(r.intersect(rays[:n]))
        assert np.array_equal(s_ids, ids[:n]) and np.array_equal(_bits(s_geom), _bits(geom[:n])), n
        s_area, s_color, s_status = r.lit_area(T[:n], check=False)
        assert np.array_equal(_bits(s_area), _bits(area[:n])) and np.array_equal(_bits(s_color), _bits(color[:n])), n
        assert np.array_equal(s_status, status[:n]), n


# 8 ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_optional_outputs_and_alignment(gpu, c2_batch):
    """NULL optional outputs leave their buffers alone; a device output pointer that is only
    8-byte aligned gives the same bits."""
    import torch
    r, rays, full = c2_batch
    ids, geom, T, area, color, status = full
    n, m, L = 1000, min(1000, len(T)), area.shape[1]
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays[:n].copy()).to(dev)
    d_T = torch.from_numpy(T[:m].copy()).to(dev)
    POISON = -777.25

    def fresh(count, dtype=torch.float64):
        return torch.full((count + 1,), POISON if dtype == torch.float64 else -777, dtype=dtype, device=dev)
    # intersect: each output alone, and geom one double off
    d_ids, d_geom = fresh(3 * n, torch.int32), fresh(13 * n)
    r.intersect_device(n, d_rays.data_ptr(), d_ids.data_ptr(), None)
    r.intersect_device(n, d_rays.data_ptr(), None, d_geom.data_ptr() + 8)
    torch.cuda.synchronize()
    assert np.array_equal(d_ids.cpu().numpy()[:3 * n].reshape(n, 3), ids[:n]) and d_ids[3 * n].item() == -777
    g = d_geom.cpu().numpy()
    assert g[0] == POISON and np.array_equal(_bits(g[1:].reshape(n, 13)), _bits(geom[:n]))
    d_geom = fresh(13 * n)
    r.intersect_device(n, d_rays.data_ptr(), None, d_geom.data_ptr())
    torch.cuda.synchronize()
    g = d_geom.cpu().numpy()
    assert g[13 * n] == POISON and np.array_equal(_bits(g[:13 * n].reshape(n, 13)), _bits(geom[:n]))
    # lit_area: no colour and no status; area one double off
    d_area, d_color, d_status = fresh(m * L), fresh(3 * m * L), fresh(m, torch.int32)
    r.lit_area_device(m, d_T.data_ptr(), None, d_area.data_ptr() + 8, None, None)
    torch.cuda.synchronize()
    a = d_area.cpu().numpy()
    assert a[0] == POISON and np.array_equal(_bits(a[1:].reshape(m, L)), _bits(area[:m]))
    assert (d_color.cpu().numpy() == POISON).all() and (d_status.cpu().numpy() == -777).all()
    d_area = fresh(m * L)
    r.lit_area_device(m, d_T.data_ptr(), None, d_area.data_ptr(), d_color.data_ptr(), d_status.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_area.cpu().numpy()[:m * L].reshape(m, L)), _bits(area[:m]))
    assert np.array_equal(_bits(d_color.cpu().numpy()[:3 * m * L].reshape(m, L, 3)), _bits(color[:m]))
    assert np.array_equal(d_status.cpu().numpy()[:m], status[:m]) and d_area[m * L].item() == POISON
    # the host form with the optional outputs NULL
    h_area = np.empty((m, L))
    assert r.lib.rtx_lit_area(r.h, m, _dp(T[:m].copy()), None, _dp(h_area), None, None) == 0
    assert np.array_equal(_bits(h_area), _bits(area[:m]))
    h_ids = np.empty((n, 3), np.int32)
    assert r.lib.rtx_intersect(r.h, n, _dp(rays[:n].copy()), _i32p(h_ids), None) == 0
    assert np.array_equal(h_ids, ids[:n])


@pytest.mark.gpu
def test_invalid_arguments(gpu, c2_batch):
    r, rays, full = c2_batch
    lib, h = r.lib, r.h
    ry = rays[:4].copy()
    T = np.zeros((4, 3))
    li = np.ones((4, 4))
    ids, geom = np.full((4, 3), 7, np.int32), np.full((4, 13), 7.0)
    area, color, st = np.full((4, 8), 7.0), np.full((4, 8, 3), 7.0), np.full(4, 7, np.int32)
    # n == 0: RTX_OK, nothing touched, whatever the pointers
    assert lib.rtx_intersect(h, 0, None, None, None) == 0
    assert lib.rtx_intersect(h, 0, _dp(ry), _i32p(ids), _dp(geom)) == 0
    assert lib.rtx_lit_area(h, 0, None, None, None, None, None) == 0
    assert lib.rtx_lit_area(h, 0, _dp(T), None, _dp(area), _dp(color), _i32p(st)) == 0
    assert lib.rtx_intersect_device(h, 0, None, None, None, None) == 0
    assert lib.rtx_lit_area_device(h, 0, None, None, None, None, None, None) == 0
    assert (ids == 7).all() and (geom == 7).all() and (area == 7).all() and (color == 7).all() and (st == 7).all()
    bad = [
        lib.rtx_intersect(h, -1, _dp(ry), _i32p(ids), _dp(geom)),          # n < 0
        lib.rtx_intersect(None, 4, _dp(ry), _i32p(ids), _dp(geom)),        # no context
        lib.rtx_intersect(h, 4, None, _i32p(ids), _dp(geom)),              # no rays
        lib.rtx_intersect(h, 4, _dp(ry), None, None),                      # both outputs NULL
        lib.rtx_intersect_device(h, -1, None, None, None, None),
        lib.rtx_intersect_device(None, 4, None, None, None, None),
        lib.rtx_intersect_device(h, 4, None, None, None, None),
        lib.rtx_lit_area(h, -1, _dp(T), None, _dp(area), None, None),
        lib.rtx_lit_area(None, 4, _dp(T), None, _dp(area), None, None),
        lib.rtx_lit_area(h, 4, None, None, _dp(area), None, None),         # no targets
        lib.rtx_lit_area(h, 4, _dp(T), None, None, _dp(color), _i32p(st)),  # no area
        lib.rtx_lit_area(h, 4, _dp(T), _dp(li), _dp(area), _dp(color), None),   # explicit lights with a colour
        lib.rtx_lit_area_device(h, -1, None, None, None, None, None, None),
        lib.rtx_lit_area_device(None, 4, None, None, None, None, None, None),
        lib.rtx_lit_area_device(h, 4, None, None, None, None, None, None),
    ]
    assert bad == [EINVAL] * len(bad), bad
    assert (ids == 7).all() and (geom == 7).all() and (area == 7).all() and (color == 7).all() and (st == 7).all()
    # a context without a scene
    ctx = C.c_void_p()
    assert lib.rtx_context_create(0, C.byref(ctx)) == 0
    assert lib.rtx_intersect(ctx, 4, _dp(ry), _i32p(ids), _dp(geom)) == EINVAL
    assert lib.rtx_lit_area(ctx, 4, _dp(T), None, _dp(area), None, None) == EINVAL
    lib.rtx_context_destroy(ctx)
    r.sync()


@pytest.mark.gpu
def test_scene_without_camera(gpu, c2_batch):
    """A context with a scene and no camera answers both queries."""
    from raytracing_rb_amd import config
    r, rays, full = c2_batch
    ids, geom, T, area, color, status = full
    sd, _ = config.load_scene(*_paths("c2"))
    lib = r.lib
    ctx = C.c_void_p()
    assert lib.rtx_context_create(0, C.byref(ctx)) == 0
    assert lib.rtx_scene_upload(ctx, C.byref(sd.desc)) == 0
    n = 300
    g_ids, g_geom = np.empty((n, 3), np.int32), np.empty((n, 13))
    assert lib.rtx_intersect(ctx, n, _dp(rays[:n].copy()), _i32p(g_ids), _dp(g_geom)) == 0
    g_area, g_color, g_st = np.empty((n, area.shape[1])), np.empty((n, area.shape[1], 3)), np.empty(n, np.int32)
    assert lib.rtx_lit_area(ctx, n, _dp(T[:n].copy()), None, _dp(g_area), _dp(g_color), _i32p(g_st)) == 0
    lib.rtx_context_destroy(ctx)
    assert np.array_equal(g_ids, ids[:n]) and np.array_equal(_bits(g_geom), _bits(geom[:n]))
    assert np.array_equal(_bits(g_area), _bits(area[:n])) and np.array_equal(_bits(g_color), _bits(color[:n]))
    assert np.array_equal(g_st, status[:n])


@pytest.mark.gpu
def test_world_methods(gpu):
    """api.World#intersect / #lit_area / #local_lights through a Camera's renderer."""
    from raytracing_rb_amd import api
    rays, ids, geom, _ = _table("mix")
    T, (area, color, calls, raised) = _table_targets("mix")
    world = api.World(_paths("mix")[0])
    api.Camera(world, _paths("mix")[1], width=16, height=8)
    hit = np.nonzero(ids[:, 0] >= 0)[0]
    for k in (hit[0], hit[len(hit) // 2], int(np.nonzero(ids[:, 0] < 0)[0][0])):
        obj, inter, direction, delta, data = world.intersect(api.Ray(list(rays[k, :3]), list(rays[k, 3:])))
        if ids[k, 0] < 0:
            assert (obj, inter, direction, delta, data) == (None,) * 5
            continue
        assert obj == ids[k, 0] and direction == ("in", "out")[ids[k, 1]] and data == (None if ids[k, 2] < 0 else ids[k, 2])
        assert inter.to_a() == geom[k, 1:4].tolist() and delta.to_a() == geom[k, 10:13].tolist()
    free = np.nonzero((calls == 0).all(axis=1))[0]
    for j in (free[0], free[-1]):
        ll = world.local_lights(api.Vec3(*T[j]))
        assert [k for k, _ in ll] == [k for k in range(area.shape[1]) if area[j, k] > 0]
        for k, col in ll:
            assert np.abs(np.array(col.to_a()) - color[j, k]).max() <= TOL
        lt = _oracle_world(*_paths("mix")).lights[0]
        assert world.lit_area(api.Vec3(*T[j]), lt.position.to_a(), lt.radius) == area[j, 0]


# 9 ---------------------------------------------------------------------------
def test_symbols_and_signatures():
    from raytracing_rb_amd import _abi
    P, I, DP, IP = C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    sig = {n: (r, a) for n, r, a in _abi.SIGNATURES}
    assert sig["rtx_intersect_device"] == (I, [P, I, P, P, P, P])
    assert sig["rtx_intersect"] == (I, [P, I, DP, IP, DP])
    assert sig["rtx_lit_area_device"] == (I, [P, I, P, P, P, P, P, P])
    assert sig["rtx_lit_area"] == (I, [P, I, DP, DP, DP, DP, IP])
    lib = _abi.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.rtx_intersect(None, 1, None, None, None) == EINVAL
    assert lib.rtx_lit_area(None, 1, None, None, None, None, None) == EINVAL
    rb = open(os.path.join(ROOT, "ext", "rtx", "lib", "rtx.rb")).read()
    for name in NAMES:
        assert "extern 'int %s(" % name in rb, name


def test_world_methods_need_a_camera():
    from raytracing_rb_amd import api
    world = api.World(_paths("mix")[0])
    for name in ("intersect", "lit_area", "local_lights"):
        assert callable(getattr(world, name))
    with pytest.raises(RuntimeError):
        world.intersect(api.Ray([1.0, 0.0, 0.0], [0.0, 0.0, 0.0]))
    with pytest.raises(RuntimeError):
        world.lit_area(api.Vec3(0.0, 0.0, 0.0), api.Vec3(0.0, 0.0, 5.0), 1.0)
    with pytest.raises(RuntimeError):
        world.local_lights(api.Vec3(0.0, 0.0, 0.0))
