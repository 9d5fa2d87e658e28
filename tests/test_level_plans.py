"""The bounce-level engine's launch plan (csrc/rtx_plan.h), on the host.

tests/golden/level_plans.json holds, per row of plan_scenes.ROWS, the packed plan
that tools/scene_dump.cpp --plan computes for the row's world with default options:
the arithmetic the launcher itself runs (rtx_levels.hip launch_level_bs calls the same
level_plan).  tests/test_gpu_plans.py renders every row and holds the launcher's own
record (option lv_plan_last) to the same number.  Here: the tool still gives the
committed plans, the table covers the plan's branches, a world of 33 lights is
refused, every row renders without a raise in the C oracle, and the worlds of
several highlights on one ray are what test_gpu_plans.py takes them for."""
import json
import os
import shutil

import numpy as np
import pytest

import plan_scenes
from conftest import GOLDEN

with open(os.path.join(GOLDEN, "level_plans.json")) as _f:
    TABLE = json.load(_f)
EINVAL = 6
LIN_LDS, BVH_LDS, BVH_MIX, BVH_LDSX, BVH_QLDS = 0, 2, 4, 5, 6       # SphMode (rtx_plan.h)
RING_FULL, RING_COMPACT = 11, 5
XR_BUF, XR_WALK = 1, 2
LDS_TOTAL = 160 * 1024


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    return plan_scenes.build_tool(tmp_path_factory.mktemp("plan_tool"))


def test_the_tool_gives_the_committed_plans(tool, tmp_path):
    assert [(r["name"], r["n_sphere"], r["n_light"], r["around"], r["pt"], r["depth"]) for r in TABLE] == list(plan_scenes.ROWS)
    got = plan_scenes.table(tool, tmp_path)
    for want, row in zip(TABLE, got):
        assert row["scalars"] == want["scalars"], row["name"]
        assert row["plan"] == want["plan"], (row["name"], plan_scenes.unpack_plan(row["plan"]),
                                             plan_scenes.unpack_plan(want["plan"]))
        assert row == want


def test_the_table_covers_the_branches():
    rows = {r["name"]: dict(plan_scenes.unpack_plan(r["plan"]), **r["scalars"]) for r in TABLE}
    kinds = {(p["mode"], p["ring"]) for p in rows.values()}
    # every sphere mode levels_auto_mode returns by default, with each ring it can have
    assert {(BVH_LDSX, RING_FULL), (BVH_LDS, RING_FULL), (BVH_LDS, RING_COMPACT), (BVH_QLDS, RING_COMPACT),
            (BVH_MIX, RING_COMPACT), (LIN_LDS, RING_FULL)} == kinds
    # levels_auto_mode returns SPH_BVH_LDSX only where the full ring fits next to it, SPH_BVH_QLDS and SPH_BVH_MIX
    # only after the full ring failed to fit beside the smaller SPH_BVH_LDS layout: no other pair can occur
    assert (BVH_LDSX, RING_COMPACT) not in kinds and (BVH_QLDS, RING_FULL) not in kinds and (BVH_MIX, RING_FULL) not in kinds
    # SPH_BVH_MIX by default needs q_ok 0 (a field centred on the origin: plan_scenes)
    assert [p["q_ok"] for p in rows.values() if p["mode"] == BVH_MIX] == [0]
    assert all(p["q_ok"] == 1 for p in rows.values() if p["mode"] != BVH_MIX)
    # 512 and 513 spheres of one seed: the host build's switch, under one launch plan
    a, b = rows["lds_512_l17"], rows["lds_513_l17"]
    assert (a["n_sphere"], b["n_sphere"]) == (512, 513) and a["rbuf_sphere"] == 0 and b["rbuf_sphere"] == 1
    assert b["lbuf_n"] > 0 and b["rbuf_n"] > 0 and b["xr"] == XR_WALK      # global buffers built for a mode that takes none
    assert [r["seed"] for r in TABLE if r["n_sphere"] in (512, 513)] == [plan_scenes.SEED] * 2
    # the light counts, 17 and 32 on both sides of the switch
    assert {0, 1, 2, 4, 16, 17, 32} <= {p["n_light"] for p in rows.values()}
    for nl in (17, 32):
        assert any(p["n_light"] == nl and p["n_sphere"] <= 512 for p in rows.values())
        assert any(p["n_light"] == nl and p["n_sphere"] > 512 for p in rows.values())
    # SPH_BVH_LDSX: the light buffer's three placements
    ldsx = [p for p in rows.values() if p["mode"] == BVH_LDSX]
    assert any(p["lbuf"] and p["rgate"] and p["xr"] == XR_BUF for p in ldsx)
    assert any(p["lbuf"] and not p["rgate"] and p["xr"] == XR_BUF for p in ldsx)
    assert any(p["lbuf_n"] > 0 and not p["lbuf"] and p["xr"] == XR_WALK for p in ldsx)
    # 32 lights: LBUF_MAX_WORDS / 32 = 256 words a light hold not even the 6 * 8 * 8 + 1 cell offsets of the
    # coarsest resolution, so no light buffer (hence no raise buffer) is built at all
    p = rows["ldsx_32_l32"]
    assert (p["n_light"], p["lbuf_n"], p["rbuf_n"], p["lbuf"], p["xr"]) == (32, 0, 0, 0, XR_WALK)
    # 17 lights still get one, at the coarsest resolution, staged
    p = rows["ldsx_32_l17"]
    assert (p["lbuf_n"], p["lbuf"]) == (8, 1)
    # the workgroup's claim counter finds no room: both ways a layout can end at the last byte
    full = [p for p in rows.values() if not p["sched"]]
    assert {p["mode"] for p in full} == {BVH_LDSX, BVH_LDS} and all(p["lds"] == LDS_TOTAL for p in full)
    assert all(p["lds"] <= LDS_TOTAL - 4 for p in rows.values() if p["sched"])
    # SPH_BVH_QLDS with and without the buffers
    assert {p["xr"] for p in rows.values() if p["mode"] == BVH_QLDS} == {XR_BUF, XR_WALK}
    assert sum(r["pt"] == 3 and r["depth"] == 4 for r in TABLE) == 1


def test_33_lights_are_refused(tool, tmp_path):
    (plan, line), = plan_scenes.host_plans(tool, [plan_scenes.make(32, 33, plan_scenes.SEED, tmp_path)[0]])
    assert plan is None and line.split()[:2] == ["status", str(EINVAL)], line
    (plan, _), = plan_scenes.host_plans(tool, [plan_scenes.make(32, 32, plan_scenes.SEED, tmp_path)[0]])
    assert plan is not None


@pytest.mark.parametrize("row", TABLE, ids=[r["name"] for r in TABLE])
def test_no_row_raises_in_the_oracle(oracle_lib, tmp_path, row):
    """test_gpu_plans.py compares frames: every row's frame exists, and its ground has lit and shadowed parts."""
    from raytracing_rb_amd import config
    w, c = plan_scenes.row_world(row, tmp_path)
    sd, cd = config.load_scene(w, c)
    assert (cd.width, cd.height, cd.pre_sample_times, cd.max_sample_times) == (48, 27, 2, 3)
    ref, st, rc = oracle_lib.Oracle(sd, cd).render(seed=plan_scenes.SEED)
    assert rc == 0 and not st.any()
    if row["n_light"] == 0:                      # no light: every hit spawns path-tracing children, no leaf ever
        assert not ref.any()
    else:
        assert len(np.unique(ref.reshape(-1, 3), axis=0)) > 200       # a picture, not a flat frame


def test_the_hidden_sphere_is_the_last_one(tmp_path):
    """The third world of the 512 / 513 pair: the 513 world but for its last sphere's centre."""
    a = plan_scenes.world_text(513, 17, plan_scenes.SEED).splitlines()
    b = plan_scenes.world_text(513, 17, plan_scenes.SEED, hide_last=True).splitlines()
    c = plan_scenes.world_text(512, 17, plan_scenes.SEED).splitlines()
    diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert len(a) == len(b) and len(diff) == 1 and "center" in a[diff[0]] and "s0512" in a[diff[0] - 1]
    per = len(plan_scenes.make_scenes.sphere("s", [0, 0, 0], 1.0, ([0] * 3,) * 4).splitlines())
    start = diff[0] - 3                          # the block's lines: type, properties, name, center, ...
    assert a[start].strip() == "- type: Sphere" and a[:start] == c[:start] and a[start + per:] == c[start:]
    assert plan_scenes.HIDDEN[0] < 0 and plan_scenes.HIDDEN[2] < -1 - 0.4          # behind the camera, under the ground


# ---------------------------------------------------------------- several highlights on one ray
HL_CASES = ((4, 3), (17, 9), (32, 32))          # n_light, k lights on the camera's axis


@pytest.mark.parametrize("n_light,k", HL_CASES)
def test_the_central_rays_fire_k_highlights(tmp_path, n_light, k):
    """By the Python oracle: the root rt_map of the central pixels is a highlight node (no child, k
    leaves, one per axis light, in the lights' order), its leaves sum to at most 1 a channel, and the
    frame's corner fires none."""
    from oracle import rt_ref
    w, c = plan_scenes.make_multi_highlight(n_light, k, tmp_path)
    world, cam = rt_ref.load_scene(w, c)
    assert len(world.lights) == n_light
    for x, y in ((23, 13), (24, 13), (23, 12), (24, 14)):
        for j in range(cam.pre_sample_times):
            ray = cam.lens_func(x, y, j)
            children, leaves = cam.ray_tracer.rt_map((ray, cam.trace_depth, rt_ref.Vec3(1.0, 1.0, 1.0), 1), x, y, j)
            assert children == [] and len(leaves) == k, (x, y, j, len(leaves))
            s = rt_ref.Vec3(0.0, 0.0, 0.0)
            for leaf in leaves:
                s = rt_ref.RayTracer.rt_reduce(s, leaf)                # raises above 1
            assert max(s.to_a()) <= 0.9 + 1e-12
            fired = [light for light, _ in world.high_lights(ray)]
            assert fired == world.lights[:k]
    assert world.high_lights(cam.lens_func(0, 0, 0)) == []


@pytest.mark.parametrize("n_light,k", HL_CASES)
def test_the_highlight_worlds_render_in_the_oracle(oracle_lib, tmp_path, n_light, k):
    from raytracing_rb_amd import config
    sd, cd = config.load_scene(*plan_scenes.make_multi_highlight(n_light, k, tmp_path))
    ref, st, rc = oracle_lib.Oracle(sd, cd).render(seed=1)
    assert rc == 0 and not st.any() and ref.max() <= 1.0
