"""rtx_render_pixels: Camera#render_at for a list of pixels in one call, with a
status, the variance and the sample count per pixel.

The colours must have the bits rtx_render writes for the same pixels, the
variance and the decision must be render_at's arithmetic (tests/pixel_stats.py)
over the GPU's own per-sample colours (Renderer.lens_rays -> Renderer.trace), and
the sample counts and statuses the oracle's.  The frames are 24 x 14 (tests/
test_pixels_api.py checks on the CPU that no variance of them lies within 1e-3
of the threshold); the cases sit where the call can go wrong: the engine
threshold of 64 samples a pass, chunk edges, the device-side count of the extras
pass (none, some, all pixels), keys no frame holds, raises in either pass.
"""

import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import scene_paths

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_stats  # noqa: E402
from pixel_stats import H, W  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = 6
N = W * H


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _renderer(sd, cd, options=()):
    from raytracing_rb_amd.runtime import Renderer
    r = Renderer(sd, cd, device=0)
    for k, v in dict(options).items():
        r.set_option(k, v)
    return r


def _pix(r, xy, engine=None, ran=None, seed=1):
    """(rgb, variance, status, samples) of one rtx_render_pixels call, under "trace_engine" `engine` if given."""
    if engine is not None:
        r.set_option("trace_engine", engine)
    out = r.render_pixels(xy, seed=seed, check=False)
    if engine is not None or ran is not None:
        assert r.get_option("trace_engine_last") == (engine if ran is None else ran)
    return out


def _bounds(rgb, ref, what):
    d = rgb - ref
    rms = np.sqrt((d ** 2).mean(axis=0))
    print(what, "rms", rms, "max |diff| %.3e" % np.abs(d).max())
    assert np.abs(d).max() <= 1e-6 and (rms <= 1e-4).all(), what


@functools.lru_cache(maxsize=None)
def _oracle_side(name):
    """(colours [N, 3], lens_func calls [N]) of the configuration's frame from the oracle, row-major."""
    from oracle.c_oracle import Oracle
    sd, cd = pixel_stats.load(name)
    oracle = Oracle(sd, cd)
    xy = pixel_stats.frame_xy(W, H)
    ref, st, rc = oracle.render_pixels(xy)
    assert rc == 0 and not st.any()
    counts, _ = pixel_stats.oracle_counts(oracle, xy)
    ref.setflags(write=False)
    counts.setflags(write=False)
    return ref, counts


@functools.lru_cache(maxsize=None)
def _c0_frame():
    """The c0_default frame: rtx_render's pixels row-major, and one rtx_render_pixels call over them."""
    r = _renderer(*pixel_stats.load("c0_default"))
    frame = r.render().reshape(-1, 3)
    full = _pix(r, pixel_stats.frame_xy(W, H))
    r.close()
    for a in (frame,) + full:
        a.setflags(write=False)
    return frame, full


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pixel_stats.CONFIGS))
def test_parity(gpu, oracle_lib, name):
    ref, counts = _oracle_side(name)
    sd, cd = pixel_stats.load(name)
    pre, mx = cd.pre_sample_times, cd.max_sample_times
    assert int((counts > pre).sum()) == pixel_stats.EXTRAS[name]
    r = _renderer(sd, cd)
    xy = pixel_stats.frame_xy(W, H)
    col, sst = pixel_stats.gpu_samples(r)
    assert not sst.any()
    want = pixel_stats.pixels(col, sst, cd.variant_threshold, pre, mx)
    for bvh in (0, 2):
        for lbuf in (0, 1):
            r.set_option("bvh", bvh)
            r.set_option("lbuf", lbuf)
            frame = r.render().reshape(-1, 3)
            for engine in (0, 1):
                rgb, var, st, samples = _pix(r, xy, engine)
                what = (name, bvh, lbuf, engine)
                assert not st.any(), what
                assert np.array_equal(samples, counts), (what, np.nonzero(samples != counts)[0][:5])
                assert np.array_equal(_bits(rgb), _bits(frame)), (what, np.nonzero((rgb != frame).any(axis=1))[0][:5])
                assert np.array_equal(_bits(var), _bits(want[1])), what
                assert np.array_equal(_bits(rgb), _bits(want[0])), what
                _bounds(rgb, ref, what)
                if engine == 1:                                     # level 0: the samples traced, and no more
                    assert r.level_stats()["rays"][0] == int(samples.sum()), (what, r.level_stats())
    r.close()


# 2 ---------------------------------------------------------------------------
def test_max_equal_pre_with_the_test_firing(gpu):
    """C2's own camera (pre = max = 4): a firing pixel takes no extra sample, its colour is (mean * 4 + 0) / 4
    as in the reference.  170 of the 336 pixels are flat (variance 0: sky)."""
    from raytracing_rb_amd import config
    sd, cd = config.load_scene(*scene_paths("c2"), camera_overrides=dict(width=W, height=H))
    assert cd.pre_sample_times == cd.max_sample_times == 4
    r = _renderer(sd, cd)
    frame = r.render().reshape(-1, 3)
    col, sst = pixel_stats.gpu_samples(r)
    want = pixel_stats.pixels(col, sst, cd.variant_threshold, 4, 4)
    for engine in (0, 1):
        rgb, var, st, samples = _pix(r, pixel_stats.frame_xy(W, H), engine)
        assert not st.any() and (samples == 4).all()
        assert np.array_equal(_bits(rgb), _bits(frame))
        assert np.array_equal(_bits(var), _bits(want[1])) and np.array_equal(_bits(rgb), _bits(want[0]))
        assert int((var == 0).sum()) == 170
        assert (var >= cd.variant_threshold).sum() > 0             # the test fires on this frame
    r.close()


# 3 ---------------------------------------------------------------------------
def _list(n):
    """n frame pixels: a fixed permutation of the frame, repeated, with at least one duplicate from n = 2."""
    idx = np.resize(np.random.default_rng(7).permutation(N), n)
    if n >= 2:
        idx[n // 2] = idx[0]
    return idx


@pytest.mark.parametrize("n", (1, 21, 22, 64, 65, 257, 4097))
def test_list_shapes(gpu, n):
    """With pre 3, 21 and 22 pixels put the pre pass on either side of the 64 samples from which "trace_engine"
    -1 runs the bounce levels; 4,097 is the frame repeated."""
    frame, full = _c0_frame()
    r = _renderer(*pixel_stats.load("c0_default"))
    idx = _list(n)
    xy = pixel_stats.frame_xy(W, H)[idx]
    for engine, ran in ((-1, 1 if 3 * n >= 64 else 0), (0, 0), (1, 1)):
        rgb, var, st, samples = _pix(r, xy, engine, ran)
        assert np.array_equal(_bits(rgb), _bits(frame[idx])), (n, engine, np.nonzero((rgb != frame[idx]).any(axis=1))[0][:5])
        assert np.array_equal(_bits(var), _bits(full[1][idx])), (n, engine)
        assert not st.any() and np.array_equal(samples, full[3][idx]), (n, engine)
        if engine == 1:                                             # level 0: the samples traced, and no more
            assert r.level_stats()["rays"][0] == int(samples.sum()), (n, r.level_stats())
    r.close()


def test_optional_outputs_and_alignment(gpu):
    """variance and info NULL, each and both; d_rgb 8 bytes off 16-byte alignment; nothing written past a buffer."""
    import torch
    frame, full = _c0_frame()
    r = _renderer(*pixel_stats.load("c0_default"))
    idx = _list(257)
    n = len(idx)
    d_xy = torch.from_numpy(pixel_stats.frame_xy(W, H)[idx]).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for want_var, want_info in ((False, True), (True, False), (False, False), (True, True)):
        raw = torch.zeros(3 * n + 4, dtype=torch.float64, device="cuda")
        off = 1 if raw.data_ptr() % 16 == 0 else 0
        d_rgb = raw[off:off + 3 * n]
        assert d_rgb.data_ptr() % 16 == 8
        d_var = torch.zeros(n + 2, dtype=torch.float64, device="cuda") if want_var else None
        d_info = torch.zeros(2 * n + 2, dtype=torch.int32, device="cuda") if want_info else None
        r.render_pixels_device(d_xy, d_rgb, d_var, d_info, stream=stream, n=n)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(d_rgb.cpu().numpy().reshape(-1, 3)), _bits(frame[idx])), (want_var, want_info)
        assert raw[3 * n + off:].sum().item() == 0 and (off == 0 or raw[0].item() == 0)
        if want_var:
            v = d_var.cpu().numpy()
            assert np.array_equal(_bits(v[:n]), _bits(full[1][idx])) and (v[n:] == 0).all()
        if want_info:
            i = d_info.cpu().numpy()
            assert not i[:2 * n:2].any() and np.array_equal(i[1:2 * n:2], full[3][idx]) and (i[2 * n:] == 0).all()
    r.sync()
    r.close()


@pytest.mark.parametrize("which", ("none", "all"))
def test_no_pixel_and_every_pixel_takes_extras(gpu, which):
    """The extras pass with a live count of zero (the mix frame under its own threshold: no pixel fires, checked on
    the CPU) and of its whole capacity (variant_threshold 0 on c0_default)."""
    from raytracing_rb_amd import config
    if which == "none":
        sd, cd = config.load_scene(*scene_paths("mix"), camera_overrides=dict(width=W, height=H))
    else:
        sd, cd = pixel_stats.load("c0_default", variant_threshold=0.0)
    r = _renderer(sd, cd)
    frame = r.render().reshape(-1, 3)
    xy = pixel_stats.frame_xy(W, H)
    for engine in (0, 1):
        rgb, var, st, samples = _pix(r, xy, engine)
        assert not st.any()
        assert (samples == (cd.pre_sample_times if which == "none" else cd.max_sample_times)).all()
        assert np.array_equal(_bits(rgb), _bits(frame)), (which, engine)
        if engine == 1:
            assert r.level_stats()["rays"][0] == int(samples.sum())
    r.close()


# 4 ---------------------------------------------------------------------------
def test_coordinates_no_frame_holds(gpu, oracle_lib):
    """Any int32 x and y: lens_func checks no bounds.  mix with aperture 0 (every lens ray is then pure
    arithmetic, the oracle's bits: checked here on the frame's own pixels), so that the GPU's sample colours can
    be had for keys Renderer.lens_rays refuses."""
    from oracle.c_oracle import Oracle
    sd, cd = pixel_stats.load("mix", aperture_radius=0.0)
    pre, mx = cd.pre_sample_times, cd.max_sample_times
    odd = [(-1, 3), (-2 ** 31, 5), (4, -5), (W + 3, 2), (-1, -5), (-7, H + 2)]
    inside = pixel_stats.frame_xy(W, H)[_list(40)]
    xy = np.concatenate([inside[:13], odd[:2], inside[13:30], odd[2:4], inside[30:], odd[4:]]).astype(np.int32)
    oracle = Oracle(sd, cd)
    ref, ost, _ = oracle.render_pixels(xy)
    counts, _ = pixel_stats.oracle_counts(oracle, xy)
    assert not ost.any() and (counts > pre).any() and (counts == pre).any()
    ocol, _, rays = pixel_stats.oracle_samples(oracle, xy)
    r = _renderer(sd, cd)
    for j in range(mx):                                             # the premise: the GPU's lens rays are the oracle's
        mine = r.lens_rays(sample=j).reshape(-1, 6)
        k = [i for i, (x, y) in enumerate(xy) if 0 <= x < W and 0 <= y < H]
        assert np.array_equal(_bits(mine[xy[k, 1] * W + xy[k, 0]]), _bits(rays[k, j]))
    keys = np.array([[(x, y, j) for j in range(mx)] for x, y in xy], np.int32).reshape(-1, 3)
    col, sst = r.trace(rays.reshape(-1, 6), keys, check=False)
    want = pixel_stats.pixels(col.reshape(-1, mx, 3), sst.reshape(-1, mx), cd.variant_threshold, pre, mx)
    for engine in (0, 1):
        rgb, var, st, samples = _pix(r, xy, engine)
        assert np.array_equal(st, ost) and np.array_equal(samples, counts), engine
        _bounds(rgb, ref, ("odd coordinates", engine))
        assert np.array_equal(_bits(rgb), _bits(want[0])) and np.array_equal(_bits(var), _bits(want[1])), engine
        if engine == 1:                                             # a negative x: those trees go to the lanes engine
            stats = r.level_stats()
            assert stats["redo"] == int(samples[xy[:, 0] < 0].sum()), stats
            assert stats["rays"][0] == int(samples.sum()), stats
    r.close()


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [
    dict(lv_batch=512), dict(lv_batch=64), dict(lv_batch=1), dict(lv_stage_pct=5, lv_floor=0),
    dict(lv_rec_pct=101, lv_floor=0), dict(lv_batch=1000, lv_stage_pct=20, lv_rec_pct=150, lv_floor=0),
    dict(lv_stage_pct=5, lv_floor=0, lv_redo_blocks=1), dict(lv_stage_pct=5, lv_floor=0, lv_redo_blocks=0),
])
def test_chunks_and_overflow_change_no_bit(gpu, opts):
    """The option sets of tests/test_gpu_levels.py's test_levels_batches_and_overflow_change_no_bit, and "lv_batch"
    64: the list in chunks of lv_batch / max(pre, max - pre) pixels (c0_default: 7 extra samples a pixel), and
    the level buffers overflowing into the lanes engine.  Level 0 of rtx_level_stats, summed over both passes
    of every chunk, is the samples taken."""
    frame, full = _c0_frame()
    r = _renderer(*pixel_stats.load("c0_default"), options=opts)
    xy = pixel_stats.frame_xy(W, H)
    for engine in (1, 0):
        rgb, var, st, samples = _pix(r, xy, engine)
        assert np.array_equal(_bits(rgb), _bits(frame)), (opts, engine)
        assert np.array_equal(_bits(var), _bits(full[1])) and np.array_equal(samples, full[3]) and not st.any()
        if engine == 1:
            stats = r.level_stats()
            assert stats["rays"][0] == int(samples.sum()), (opts, stats)
            if "lv_stage_pct" in opts or "lv_rec_pct" in opts:
                assert stats["redo"] > 0, stats                    # the overflow path ran
    r.close()


# 6 ---------------------------------------------------------------------------
def _render_raw(r):
    """(rtx_status, the buffer's bits) of rtx_render of the whole frame: a raising frame fills its buffer too."""
    out = np.zeros((r.height, r.width, 3), np.float64)
    st = r.lib.rtx_render(r.h, 0, 0, r.width, r.height, 1, out.ctypes.data_as(C.POINTER(C.c_double)), r.width * 3)
    return st, _bits(out).copy()


@pytest.mark.parametrize("fillers", (0, 40))
@pytest.mark.parametrize("case", ("pixel_A_back", "pixel_B_front", "pixel_A_far"))
def test_raises(gpu, oracle_lib, tmp_path, case, fillers):
    """The pixel cases of tests/test_raises.py (24 x 16, one pixel whose local_lights raises Math::DomainError):
    with the scene's camera (pre = max = 1) the pre pass raises; with pre 2, max 4 and variant_threshold 0 every
    pixel takes the extras and, the aperture being 0, every sample of the pixel raises: sample 0 reports."""
    import test_raises
    from oracle.c_oracle import Oracle
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import RtxError
    assert case in test_raises.PIXEL_CASES
    test_raises._pixel_scene(tmp_path, case, fillers=fillers)
    paths = (str(tmp_path / "w.yml"), str(tmp_path / "c.yml"))
    for ov in ({}, dict(pre_sample_times=2, max_sample_times=4, variant_threshold=0.0)):
        sd, cd = config.load_scene(*paths, camera_overrides=ov)
        assert cd.aperture_radius == 0.0
        pre, mx = cd.pre_sample_times, cd.max_sample_times
        _, omap, rc = Oracle(sd, cd).render()
        assert rc == 3 and (omap != 0).sum() == 1
        xy = pixel_stats.frame_xy(cd.width, cd.height)
        bad = int(np.nonzero(omap.reshape(-1))[0][0])
        r = _renderer(sd, cd)
        before = _render_raw(r)
        assert before[0] == 3
        col, sst = pixel_stats.gpu_samples(r)
        want = pixel_stats.pixels(col, sst, cd.variant_threshold, pre, mx)
        ok = np.arange(len(xy)) != bad
        for engine in (0, 1):
            rgb, var, st, samples = _pix(r, xy, engine)
            assert np.array_equal(st.reshape(cd.height, cd.width), omap), (ov, engine)
            assert st[bad] == 3 and samples[bad] == 1 and np.isnan(rgb[bad]).all() and np.isnan(var[bad])
            assert (samples[ok] == mx).all()
            assert np.array_equal(_bits(rgb[ok]), _bits(want[0][ok])), (ov, engine)
            assert np.array_equal(_bits(var[ok]), _bits(want[1][ok])), (ov, engine)
            assert np.array_equal(st, want[2]) and np.array_equal(samples, want[3])
            with pytest.raises(RtxError) as e:                      # the host form names the pixel's index
                r.render_pixels(xy)
            assert e.value.kind == "domain"
            assert "at pixel %d (%d, %d)" % (bad, xy[bad, 0], xy[bad, 1]) in str(e.value), str(e.value)
            r.sync()                                                # nothing was recorded in rtx_sync's state
        after = _render_raw(r)
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
        r.close()


def test_every_pixel_takes_extras_on_mix(gpu):
    """k_pixel_finish's arithmetic on every pixel of a frame with Monte-Carlo children (mix, variant_threshold
    0): the restatement over the GPU's sample colours, and the render."""
    sd, cd = pixel_stats.load("mix", variant_threshold=0.0)
    r = _renderer(sd, cd)
    col, sst = pixel_stats.gpu_samples(r)
    want = pixel_stats.pixels(col, sst, 0.0, cd.pre_sample_times, cd.max_sample_times)
    rgb, var, st, samples = _pix(r, pixel_stats.frame_xy(W, H), 1)
    assert (samples == cd.max_sample_times).all() and not st.any()
    assert np.array_equal(_bits(rgb), _bits(want[0])) and np.array_equal(_bits(var), _bits(want[1]))
    assert np.array_equal(_bits(rgb), _bits(r.render().reshape(-1, 3)))
    r.close()


# 7 ---------------------------------------------------------------------------
def test_posed_scene(gpu, tmp_path):
    """fuzz_scenes' posed seed 2: scale 40, offset 80,000, max_distance binding; a threshold at which pixels of it
    take extra samples."""
    import fuzz_scenes
    from raytracing_rb_amd import config
    assert fuzz_scenes.posed_parameters(2)[0] == 40.0
    w, c = fuzz_scenes.make_posed(2, tmp_path, W, H, bind_distance=True)
    sd, cd = config.load_scene(w, c, camera_overrides=dict(variant_threshold=1e-7))
    assert cd.max_sample_times > cd.pre_sample_times
    r = _renderer(sd, cd)
    frame = r.render(seed=2).reshape(-1, 3)
    for engine in (0, 1):
        rgb, var, st, samples = _pix(r, pixel_stats.frame_xy(W, H), engine, seed=2)
        assert not st.any() and np.array_equal(_bits(rgb), _bits(frame)), engine
        assert (samples > cd.pre_sample_times).any() and (samples == cd.pre_sample_times).any()
    r.close()


# 8 ---------------------------------------------------------------------------
def test_streams_and_back_to_back_calls(gpu):
    import torch
    frame, full = _c0_frame()
    r = _renderer(*pixel_stats.load("c0_default"))
    xy = pixel_stats.frame_xy(W, H)
    a, b = _list(257), _list(65)[::-1].copy()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = [torch.from_numpy(xy[i]).cuda() for i in (a, b)]
        rgb = [torch.empty((len(i), 3), dtype=torch.float64, device="cuda") for i in (a, b)]
        info = [torch.empty((len(i), 2), dtype=torch.int32, device="cuda") for i in (a, b)]
        for k in range(2):                                           # two calls back to back, no sync between
            r.render_pixels_device(d[k], rgb[k], None, info[k], stream=s.cuda_stream)
    s.synchronize()
    for k, i in enumerate((a, b)):
        assert np.array_equal(_bits(rgb[k].cpu().numpy()), _bits(frame[i])), k
        assert np.array_equal(info[k].cpu().numpy()[:, 1], full[3][i]) and not info[k].cpu().numpy()[:, 0].any()
    r.sync()
    r.close()


def test_arguments(gpu):
    import torch
    from raytracing_rb_amd import _abi, config
    lib = _abi.load_library()
    sd, cd = pixel_stats.load("c0_default")
    r = _renderer(sd, cd)
    n = 5
    d_xy = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    d_rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    xy, rgb = np.zeros((n, 2), np.int32), np.zeros((n, 3))
    p = lambda t: C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data)   # noqa: E731
    dev, host = lib.rtx_render_pixels_device, lib.rtx_render_pixels
    assert dev(r.h, 0, 1, None, None, None, None, None) == 0 and host(r.h, 0, 1, None, None, None, None) == 0
    assert dev(r.h, -1, 1, p(d_xy), p(d_rgb), None, None, None) == EINVAL
    assert host(r.h, -1, 1, p(xy), p(rgb), None, None) == EINVAL
    assert dev(None, n, 1, p(d_xy), p(d_rgb), None, None, None) == EINVAL
    assert host(None, n, 1, p(xy), p(rgb), None, None) == EINVAL
    assert dev(r.h, n, 1, None, p(d_rgb), None, None, None) == EINVAL
    assert dev(r.h, n, 1, p(d_xy), None, None, None, None) == EINVAL
    assert host(r.h, n, 1, None, p(rgb), None, None) == EINVAL
    assert host(r.h, n, 1, p(xy), None, None, None) == EINVAL
    assert dev(r.h, n, 1, p(d_xy), p(d_rgb), None, None, None) == 0 and host(r.h, n, 1, p(xy), p(rgb), None, None) == 0
    torch.cuda.synchronize()
    r.close()
    ctx = C.c_void_p()                                             # no scene, then no camera
    assert lib.rtx_context_create(0, C.byref(ctx)) == 0
    assert dev(ctx, n, 1, p(d_xy), p(d_rgb), None, None, None) == EINVAL
    assert host(ctx, n, 1, p(xy), p(rgb), None, None) == EINVAL
    assert lib.rtx_scene_upload(ctx, C.byref(sd.desc)) == 0
    assert dev(ctx, n, 1, p(d_xy), p(d_rgb), None, None, None) == EINVAL
    assert host(ctx, n, 1, p(xy), p(rgb), None, None) == EINVAL
    lib.rtx_context_destroy(ctx)
    # a camera whose ray stack exceeds 64 entries, refused as by rtx_trace
    sd2, cd2 = pixel_stats.load("c0_default", trace_depth=40, monte_carlo_diffusion_times=1)
    r2 = _renderer(sd2, cd2)
    assert 1 + 39 * 2 > 64
    assert dev(r2.h, n, 1, p(d_xy), p(d_rgb), None, None, None) == EINVAL
    assert host(r2.h, n, 1, p(xy), p(rgb), None, None) == EINVAL
    r2.close()


def test_camera_sampling_and_the_cli_map(gpu, tmp_path):
    """Camera.sampling() against Camera.render(), Camera.render_pixels(), and `rtx a`'s picture against the map
    computed from Camera.sampling()."""
    from raytracing_rb_amd import _build, api, png
    world_yml, camera_yml = scene_paths("c0_default")
    world = api.World(world_yml)
    cam = api.Camera(world, camera_yml, width=W, height=H)
    frame = cam.render()
    rgb, var, samples, status = cam.sampling()
    assert rgb.shape == (H, W, 3) and var.shape == samples.shape == status.shape == (H, W)
    assert np.array_equal(_bits(rgb), _bits(frame)) and not status.any()
    assert np.array_equal(samples.reshape(-1), _c0_frame()[1][3])
    sub = cam.sampling(3, 2, 20, 11)
    assert np.array_equal(_bits(sub[0]), _bits(frame[2:11, 3:20])) and np.array_equal(sub[2], samples[2:11, 3:20])
    xy = [(5, 7), (0, 0), (W - 1, H - 1)]
    assert np.array_equal(_bits(cam.render_pixels(xy)), _bits(np.array([frame[y, x] for x, y in xy])))
    exe = _build.build_cli()
    out = str(tmp_path / "a.png")
    subprocess.run([exe, "a", out, world_yml, camera_yml, "--set", "width=%d" % W, "--set", "height=%d" % H],
                   check=True, timeout=120)
    img = png.decode_rgb8(out)
    ms = max(cam.desc.pre_sample_times, cam.desc.max_sample_times)
    grey = (255 * samples.astype(np.int64) // ms).astype(np.uint8)
    assert img.shape == (H, W, 3)
    for k in range(3):
        assert np.array_equal(img[..., k], grey), k
    assert len(np.unique(grey)) == 2
