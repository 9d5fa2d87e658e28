"""Batched Camera#lens_func (rtx_lens_rays; rtx_rtmap.hip k_lens_rays): the rays
camera.rb:129-151 draws for the pixels of a rectangle, against the Python
restatement of the reference (oracle/rt_ref.py Camera.lens_func).

With ``aperture_radius: 0`` the draw's cos / sin are multiplied by zero and every
value is compared on its uint64 view; with the scenes' own apertures libm's cos /
sin and the device's differ in the last bits and the rays are compared within
1e-9, the project's max-|diff| bound.
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import scene_paths

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-9
EINVAL = 6
W, H = 24, 14


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _renderer(name, **ov):
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    sd, cd = config.load_scene(*scene_paths(name), camera_overrides=ov)
    return Renderer(sd, cd, device=0)


def _oracle_rays(name, sample, x0, y0, x1, y1, **ov):
    from oracle import rt_ref
    _, cam = rt_ref.load_scene(*scene_paths(name), overrides=dict(ov))
    out = np.empty((y1 - y0, x1 - x0, 6))
    for y in range(y0, y1):
        for x in range(x0, x1):
            r = cam.lens_func(x, y, sample)
            out[y - y0, x - x0] = r.front.to_a() + r.position.to_a()
    return out


RECTS = ((0, 0, W, H), (3, 2, 20, 11), (23, 13, 24, 14), (0, 5, 24, 6), (7, 0, 8, 14))


@pytest.mark.gpu
def test_lens_rays_aperture_zero_bit_for_bit(gpu):
    """mix, every sample of the camera, the frame and ragged sub-rectangles."""
    ov = dict(width=W, height=H, aperture_radius=0.0)
    r = _renderer("mix", **ov)
    ms = max(r.camera.pre_sample_times, r.camera.max_sample_times)
    assert ms > 1
    for sample in range(ms):
        for (x0, y0, x1, y1) in RECTS if sample == 0 else RECTS[:2]:
            got = r.lens_rays(x0, y0, x1, y1, sample=sample)
            want = _oracle_rays("mix", sample, x0, y0, x1, y1, **ov)
            assert got.shape == want.shape == (y1 - y0, x1 - x0, 6)
            assert np.array_equal(_bits(got), _bits(want)), (sample, x0, y0, x1, y1)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("mix", "c2"))
def test_lens_rays_with_the_scene_aperture(gpu, name):
    ov = dict(width=W, height=H)
    r = _renderer(name, **ov)
    assert r.camera.aperture_radius > 0
    seen = []
    for sample in (0, 1):
        got = r.lens_rays(3, 2, 20, 11, sample=sample)
        want = _oracle_rays(name, sample, 3, 2, 20, 11, **ov)
        d = np.abs(got - want).max()
        print(name, sample, "max |diff| %.3e" % d)
        assert d <= TOL
        seen.append(got)
    assert not np.array_equal(seen[0][..., 3:], seen[1][..., 3:])     # the samples draw different aperture points
    r.close()


@pytest.mark.gpu
def test_intersect_of_lens_rays_equals_first_hit(gpu):
    """The returned rays through rtx_intersect: rtx_first_hit's ids and ten values, bit for bit."""
    r = _renderer("mix", width=48, height=27)
    for sample in (0, 1):
        rays = r.lens_rays(sample=sample)
        g = r.intersect(rays.reshape(-1, 6))
        fh = r.first_hit(sample=sample)
        for k in ("object", "direction", "data"):
            assert np.array_equal(g[k], fh[k].reshape(-1)), (sample, k)
        for k in ("depth", "position", "normal", "albedo"):
            assert np.array_equal(_bits(g[k]).reshape(-1), _bits(fh[k]).reshape(-1)), (sample, k)
        assert len(np.unique(fh["object"])) >= 3
    r.close()


@pytest.mark.gpu
def test_device_form_and_seed(gpu):
    import torch
    r = _renderer("c2", width=W, height=H)
    dev = torch.device("cuda", 0)
    host = r.lens_rays(3, 2, 20, 11, seed=7, sample=2)
    for off in (0, 1):                               # a 16-byte aligned buffer, and one that is 8 bytes off
        buf = torch.full((17 * 9 * 6 + 2,), -777.25, dtype=torch.float64, device=dev)
        r.lens_rays_device(buf.data_ptr() + 8 * off, seed=7, sample=2, x0=3, y0=2, x1=20, y1=11)
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        assert np.array_equal(_bits(b[off:off + 17 * 9 * 6]), _bits(host).reshape(-1)), off
        assert (b[:off] == -777.25).all() and (b[off + 17 * 9 * 6:] == -777.25).all()
    assert not np.array_equal(host, r.lens_rays(3, 2, 20, 11, seed=8, sample=2))
    r.sync()
    r.close()


@pytest.mark.gpu
def test_lens_rays_invalid_arguments(gpu):
    """rtx_first_hit's argument checks."""
    r = _renderer("c2", width=W, height=H)
    lib, h = r.lib, r.h
    ms = max(r.camera.pre_sample_times, r.camera.max_sample_times)
    buf = np.full((H, W, 6), 7.0)
    bad = [
        lib.rtx_lens_rays(None, 0, 0, W, H, 1, 0, _dp(buf)),          # no context
        lib.rtx_lens_rays(h, 0, 0, W, H, 1, 0, None),                 # no buffer
        lib.rtx_lens_rays(h, 0, 0, W + 1, H, 1, 0, _dp(buf)),         # outside the frame
        lib.rtx_lens_rays(h, 0, 0, W, H + 1, 1, 0, _dp(buf)),
        lib.rtx_lens_rays(h, -1, 0, W, H, 1, 0, _dp(buf)),
        lib.rtx_lens_rays(h, 0, -1, W, H, 1, 0, _dp(buf)),
        lib.rtx_lens_rays(h, 5, 0, 5, H, 1, 0, _dp(buf)),             # empty
        lib.rtx_lens_rays(h, 0, 9, W, 3, 1, 0, _dp(buf)),
        lib.rtx_lens_rays(h, 0, 0, W, H, 1, -1, _dp(buf)),            # sample outside [0, max samples)
        lib.rtx_lens_rays(h, 0, 0, W, H, 1, ms, _dp(buf)),
        lib.rtx_lens_rays_device(None, 0, 0, W, H, 1, 0, None, None),
        lib.rtx_lens_rays_device(h, 0, 0, W, H, 1, 0, None, None),
        lib.rtx_lens_rays_device(h, 0, 0, W + 1, H, 1, 0, C.c_void_p(buf.ctypes.data), None),
    ]
    assert bad == [EINVAL] * len(bad), bad
    assert (buf == 7.0).all()
    ctx = C.c_void_p()                               # a context without a scene or camera
    assert lib.rtx_context_create(0, C.byref(ctx)) == 0
    assert lib.rtx_lens_rays(ctx, 0, 0, 1, 1, 1, 0, _dp(buf)) == EINVAL
    lib.rtx_context_destroy(ctx)
    r.sync()
    r.close()


def test_lens_rays_symbols():
    from raytracing_rb_amd import _abi, api
    P, I, U, DP = C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(C.c_double)
    sig = {n: (r, a) for n, r, a in _abi.SIGNATURES}
    assert sig["rtx_lens_rays_device"] == (I, [P, I, I, I, I, U, I, P, P])
    assert sig["rtx_lens_rays"] == (I, [P, I, I, I, I, U, I, DP])
    lib = _abi.load_library()
    assert lib.rtx_lens_rays(None, 0, 0, 1, 1, 1, 0, None) == EINVAL
    assert callable(api.Camera.lens_rays)
