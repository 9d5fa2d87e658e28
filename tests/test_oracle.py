"""The oracle itself: C restatement vs committed goldens (made by the Python
restatement) and vs the Python restatement on fresh inputs — bit for bit."""

import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCENES
from oracle import rt_ref
from oracle.c_oracle import Oracle, lib as oracle_lib
from oracle.rng import child_path, rtx_rand
from raytracing_rb_amd import config

FRAMES = ["c1_64x36", "c0_48x27", "c2_32x18", "mix_24x14"]


def _load(name):
    z = np.load(os.path.join(GOLDEN, "frame_%s.npz" % name))      # allow_pickle=False
    return z


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _oracle_for(z):
    ov = eval(str(z["overrides"]), {})                             # our own repr() of a small dict
    sd, cd = config.load_scene(os.path.join(SCENES, str(z["world"])), os.path.join(SCENES, str(z["camera"])),
                               camera_overrides=ov)
    return Oracle(sd, cd), ov


@pytest.mark.parametrize("name", FRAMES)
def test_c_oracle_matches_golden(oracle_lib, name):
    z = _load(name)
    assert _sha(os.path.join(SCENES, str(z["world"]))) == str(z["scene_sha"]), "scene file drifted from fixture"
    o, _ = _oracle_for(z)
    fb, st, rc = o.render(seed=int(z["seed"]))
    assert np.array_equal(st, z["status"])
    assert np.array_equal(fb.view(np.uint64), z["frame"].view(np.uint64)), "C oracle != golden (bitwise)"


@pytest.mark.parametrize("world,camera,ov", [
    ("c2_world.yml", "c2_camera.yml", {"width": 20, "height": 12}),
    ("c0_world.yml", "camera.yml", {"width": 24, "height": 14}),
    ("mix_world.yml", "mix_camera.yml", {"width": 16, "height": 9}),
])
def test_python_and_c_restatements_agree_fresh_seed(oracle_lib, world, camera, ov):
    seed = 12345
    sd, cd = config.load_scene(os.path.join(SCENES, world), os.path.join(SCENES, camera), camera_overrides=ov)
    fb, st, rc = Oracle(sd, cd).render(seed=seed)
    _, cam = rt_ref.load_scene(os.path.join(SCENES, world), os.path.join(SCENES, camera), seed=seed, overrides=ov)
    py = np.array(cam.render(), dtype=np.float64)
    assert rc == 0
    assert np.array_equal(py.view(np.uint64), fb.view(np.uint64))


def test_rng_contract_three_implementations(oracle_lib):
    from raytracing_rb_amd import _abi
    L = _abi.load_library()
    z = np.load(os.path.join(GOLDEN, "vectors.npz"))
    for k, v in zip(z["rng_keys"], z["rng"]):
        k = [int(a) for a in k]
        assert rtx_rand(1, *k) == v
        assert oracle_lib.lib().rto_rand(1, *k) == v
        assert L.rtx_rand(1, *k) == v
    assert 0.0 <= z["rng"].min() and z["rng"].max() < 1.0
    assert child_path(1, 2, 1) == 6 and child_path(5, 3, 2) == 28


def test_lens_and_trace_vectors(oracle_lib):
    z = np.load(os.path.join(GOLDEN, "vectors.npz"))
    assert _sha(os.path.join(SCENES, "c2_world.yml")) == str(z["scene_sha"])
    sd, cd = config.load_scene(os.path.join(SCENES, "c2_world.yml"), os.path.join(SCENES, "c2_camera.yml"))
    o = Oracle(sd, cd)
    for (x, y, j), ray in zip(z["lens_keys"], z["lens"]):
        assert np.array_equal(o.lens(int(x), int(y), int(j)), ray)
    out, st, rc = o.trace(z["lens"], z["lens_keys"])
    assert rc == 0
    assert np.array_equal(out.view(np.uint64), z["trace"].view(np.uint64))


def test_fork_baseline_equals_serial(oracle_lib):
    sd, cd = config.load_scene(os.path.join(SCENES, "c2_world.yml"), os.path.join(SCENES, "c2_camera.yml"),
                               camera_overrides={"width": 30, "height": 10})
    o = Oracle(sd, cd)
    a = o.render_fork(4, col_stride=1)
    b, st, rc = o.render()
    assert np.array_equal(a, b)
    c = o.render_fork(3, col_stride=4)
    assert np.array_equal(c[:, ::4], b[:, ::4])


def _bright_scene(tmp_path):
    """A scene violating the <= 1 bound: rt_reduce must raise (ray_tracer.rb:294-296)."""
    src = open(os.path.join(SCENES, "c1_world.yml")).read()
    src = src.replace("diffuse_rate:           [0.5, 0.5, 0.5]", "diffuse_rate:           [0.99, 0.99, 0.99]")
    src = src.replace("ambient:                [0.05, 0.05, 0.05]", "ambient:                [0.3, 0.3, 0.3]", 1)
    p = tmp_path / "bright.yml"
    p.write_text(src)
    return str(p)


def test_color_gt1_raise_site(oracle_lib, tmp_path):
    world = _bright_scene(tmp_path)
    ov = {"width": 24, "height": 14}
    sd, cd = config.load_scene(world, os.path.join(SCENES, "c1_camera.yml"), camera_overrides=ov)
    fb, st, rc = Oracle(sd, cd).render()
    assert rc == 2 and (st == 2).any()
    _, cam = rt_ref.load_scene(world, os.path.join(SCENES, "c1_camera.yml"), overrides=ov)
    pys = np.zeros_like(st)
    for x in range(24):
        for y in range(14):
            try:
                cam.render_at(x, y)
            except Exception as e:
                pys[y, x] = {"color_gt1": 2, "zero_vec": 1, "domain": 3}[e.kind]
    assert np.array_equal(pys, st)


@pytest.fixture(scope="module")
def c4_scene():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(SCENES), "tools"))
    import make_scenes
    return make_scenes.ensure_c4()


def test_c4_golden_and_python_restatement_on_sampled_pixels(oracle_lib, c4_scene):
    """C4 (4096 spheres): the committed golden (made by the C restatement) is
    reproduced bit for bit, and the pure-Python restatement agrees with the C
    one on sampled pixels (all 8 samples, depth 8)."""
    z = _load("c4_48x27")
    assert _sha(c4_scene) == str(z["scene_sha"]), "scene file drifted from fixture"
    ov = eval(str(z["overrides"]), {})
    sd, cd = config.load_scene(c4_scene, os.path.join(SCENES, "c4_camera.yml"), camera_overrides=ov)
    xy = np.array([[5, 3], [24, 13], [40, 20]], np.int32)
    ref, st, rc = Oracle(sd, cd).render_pixels(xy, seed=1)
    assert rc == 0
    assert np.array_equal(ref.view(np.uint64), z["frame"][xy[:, 1], xy[:, 0]].view(np.uint64))
    _, cam = rt_ref.load_scene(c4_scene, os.path.join(SCENES, "c4_camera.yml"), seed=1, overrides=ov)
    py = np.array([cam.render_at(int(x), int(y)).to_a() for x, y in xy], dtype=np.float64)
    assert np.array_equal(py.view(np.uint64), ref.view(np.uint64))


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_scenes_python_and_c_restatements_agree(oracle_lib, tmp_path, seed):
    """Seeded random scenes (tests/fuzz_scenes.py: spheres, planes, boxes,
    textures, mirrors, glass, refractive planes, 1-3 point / area lights,
    random sampling, depth and path tracing): the C oracle and the line-by-line
    Python restatement agree bit for bit, raise sites included."""
    import fuzz_scenes
    from oracle.rb_vec3 import RtxError
    w, c = fuzz_scenes.make(seed, tmp_path, 12, 8)
    sd, cd = config.load_scene(w, c)
    fb, st, rc = Oracle(sd, cd).render(seed=seed)
    _, cam = rt_ref.load_scene(w, c, seed=seed)
    codes = {"zero_vec": 1, "color_gt1": 2, "domain": 3}
    py = np.zeros_like(fb)
    pst = np.zeros_like(st)
    for x in range(cd.width):
        for y in range(cd.height):
            try:
                py[y, x] = cam.render_at(x, y).to_a()
            except RtxError as e:
                pst[y, x] = codes[e.kind]
    assert np.array_equal(st, pst)
    assert np.array_equal(py[st == 0].view(np.uint64), fb[st == 0].view(np.uint64))


# ---------------------------------------------------------------- posed scenes
# sha256 (first 16 hex digits) of fuzz_scenes.make(seed, dir, 48, 27)'s world + camera
# text for seeds 0-23, the textures directory written as "<textures>", taken from the
# generator before pose() was added: the 24 fuzz scenes are fixtures and stay as they are.
MAKE_SHA = (
    "133e001976256920", "3587bc20a33507f4", "665bc78d1a863f46", "1ddfd868aedb1eb7",
    "40e47be50243f2d8", "a4141fbeb26a1d4f", "10062a99d4ad150b", "332ee6504d5f532e",
    "2b8007e531187beb", "0a181ca613d24926", "612177f054f3e9bd", "0496e02b18ec5037",
    "2f5a57badddd3372", "75cf10a3e06de563", "a10ea7f0486c1fdb", "fd3c85469fc261e1",
    "cb94387ce413899d", "a95dbdea57ec0bf3", "1a644837f875c496", "8152b872179c1bb7",
    "bdd8988c29d5a997", "d9443c053c72e155", "9353dd2f8e04217a", "32e2c6ece51143c9",
)


def test_fuzz_scene_files_unchanged(tmp_path):
    import fuzz_scenes
    for seed, sha in enumerate(MAKE_SHA):
        h = hashlib.sha256()
        for p in fuzz_scenes.make(seed, tmp_path, 48, 27):
            with open(p) as f:
                h.update(f.read().replace(fuzz_scenes.TEXTURES, "<textures>").encode())
        assert h.hexdigest()[:16] == sha, seed


def test_posed_seeds_cover_every_combination():
    import fuzz_scenes
    seeds = fuzz_scenes.POSED_SEEDS
    assert len(seeds) == 12 and [s % 12 for s in seeds] == list(range(12))
    params = [fuzz_scenes.posed_parameters(s) for s in seeds]
    assert {(sc, off / sc) for sc, off, _ in params} == {(sc, off) for sc in fuzz_scenes.POSED_SCALES
                                                         for off in fuzz_scenes.POSED_OFFSETS}
    assert [b for _, _, b in params] == [(k // 2) % 2 == 1 for k in range(12)]


def test_pose_maps_points_directions_and_lengths(tmp_path):
    """pose() on mix_world.yml: every point is t + scale Q p with one orthonormal Q
    and one t, directions keep their angles and take lengths in [0.4, 2.5], lengths
    scale, the camera's up is neither unit nor perpendicular, intrinsics stay."""
    import fuzz_scenes
    src = (os.path.join(SCENES, "mix_world.yml"), os.path.join(SCENES, "mix_camera.yml"))
    scale = 40.0
    w, c = fuzz_scenes.pose(src[0], src[1], tmp_path, 5, scale, 2000.0, True)
    a, b = config.load_yaml(src[0]), config.load_yaml(w)
    ca, cb = config.load_yaml(src[1]), config.load_yaml(c)
    assert b["max_distance"] == 9.0 * scale
    pts, dirs = [], []
    for ia, ib in zip(a["lights"] + a["world_objects"], b["lights"] + b["world_objects"]):
        pa, pb = ia["properties"], ib["properties"]
        assert list(pa) == list(pb)
        for k in pa:
            if k in fuzz_scenes.POINT_KEYS:
                pts.append((pa[k], pb[k]))
            elif k in fuzz_scenes.DIRECTION_KEYS:
                dirs.append((pa[k], pb[k]))
            elif k in fuzz_scenes.LENGTH_KEYS:
                assert pb[k] == pa[k] * scale, k
            elif k == "texture_file_path":
                assert os.path.isabs(pb[k]) and os.path.exists(pb[k])
            else:
                assert pb[k] == pa[k], k
    pts.append((ca["position"], cb["position"]))
    dirs.append((ca["front"], cb["front"]))
    P, P2 = np.array([p for p, _ in pts]), np.array([p for _, p in pts])
    D, D2 = np.array([d for d, _ in dirs]), np.array([d for _, d in dirs])
    t = P2[-1]                                                    # the camera was at the origin
    assert np.abs(t).max() <= 2000.0 and np.abs(t).max() > 1.0
    Q = np.linalg.lstsq(P * scale, P2 - t, rcond=None)[0].T
    assert np.allclose(Q.dot(Q.T), np.eye(3), atol=1e-9) and np.linalg.det(Q) > 0
    ln = np.linalg.norm(D2, axis=1) / np.linalg.norm(D, axis=1)
    assert (ln >= 0.4).all() and (ln <= 2.5).all() and len(set(ln.round(9))) == len(ln)
    assert np.allclose(D2 / np.linalg.norm(D2, axis=1)[:, None], (D / np.linalg.norm(D, axis=1)[:, None]).dot(Q.T),
                       atol=1e-9)
    up, front = np.array(cb["up"]), np.array(cb["front"])
    cos = up.dot(front) / np.linalg.norm(up) / np.linalg.norm(front)
    assert abs(cos - 0.3 / np.sqrt(1.09)) < 1e-9
    for k in ca:
        if k not in ("position", "up", "front"):
            assert cb[k] == ca[k], k


@pytest.mark.parametrize("k", range(12))
def test_posed_scenes_python_and_c_restatements_agree(oracle_lib, tmp_path, k):
    """make_posed (a random rotation, scale 0.02 / 1 / 40, offset up to 1e5 scale,
    non-unit and non-perpendicular bases, max_distance inside the geometry on half
    of them): the two restatements agree bit for bit off the origin pose, raise
    sites included."""
    import fuzz_scenes
    from oracle.rb_vec3 import RtxError
    seed = fuzz_scenes.POSED_SEEDS[k]
    w, c = fuzz_scenes.make_posed(seed, tmp_path, 12, 8)
    sd, cd = config.load_scene(w, c)
    fb, st, rc = Oracle(sd, cd).render(seed=seed)
    _, cam = rt_ref.load_scene(w, c, seed=seed)
    codes = {"zero_vec": 1, "color_gt1": 2, "domain": 3}
    py = np.zeros_like(fb)
    pst = np.zeros_like(st)
    for x in range(cd.width):
        for y in range(cd.height):
            try:
                py[y, x] = cam.render_at(x, y).to_a()
            except RtxError as e:
                pst[y, x] = codes[e.kind]
    assert np.array_equal(st, pst)
    assert np.array_equal(py[st == 0].view(np.uint64), fb[st == 0].view(np.uint64))


def _distinct_from_mode(fb):
    _, counts = np.unique(np.ascontiguousarray(fb).reshape(-1, 3), axis=0, return_counts=True)
    return 1.0 - counts.max() / float(counts.sum())


@pytest.mark.parametrize("k", range(12))
def test_posed_scene_conditions(oracle_lib, tmp_path, k):
    """What the posed GPU tests rely on, by the C oracle alone at their 48x27: the
    scene is still in view (>= 20 % of the pixels differ from the modal colour), at
    most a quarter of the pixels raise, and a binding max_distance changes >= 5 %
    of the pixels against the same pose with max_distance 10000 scale."""
    import fuzz_scenes
    seed = fuzz_scenes.POSED_SEEDS[k]
    scale, offset, bind = fuzz_scenes.posed_parameters(seed)
    w, c = fuzz_scenes.make_posed(seed, tmp_path, 48, 27)
    sd, cd = config.load_scene(w, c)
    assert sd.desc.max_distance == (9.0 if bind else 10000.0) * scale
    fb, st, rc = Oracle(sd, cd).render(seed=seed)
    raising = float((st != 0).mean())
    in_view = _distinct_from_mode(fb)
    print("posed seed %d (scale %g, offset %g, bind %d): raising %.4f, distinct from the mode %.4f"
          % (seed, scale, offset, bind, raising, in_view))
    assert raising <= 0.25, raising
    assert in_view >= 0.20, in_view
    if bind:
        w2, c2 = fuzz_scenes.make_posed(seed, tmp_path, 48, 27, bind_distance=False)
        sd2, cd2 = config.load_scene(w2, c2)
        assert sd2.desc.max_distance == 10000.0 * scale
        fb2, st2, _ = Oracle(sd2, cd2).render(seed=seed)
        changed = float(((fb != fb2).any(axis=-1) | (st != st2)).mean())
        print("posed seed %d: max_distance 9 scale changes %.4f of the pixels" % (seed, changed))
        assert changed >= 0.05, changed
        assert _distinct_from_mode(fb2) >= 0.20
