"""rtx_render_pixels' interface and render_at's sampling decision (no GPU).

The header declares both calls, librtx.so exports them, and the ctypes prototypes
(raytracing_rb_amd/_abi.py) and the Fiddle externs (ext/rtx/lib/rtx.rb) agree with
the header's argument lists, as tests/test_trace_api.py checks for rtx_trace_device.

tests/pixel_stats.py restates camera.rb:70-99 over per-sample colours.  On the three
configurations of the GPU parity test (whole 24 x 14 frames) its decision, over the
oracle's own Oracle.lens -> Oracle.trace samples, equals the lens_func calls the
oracle itself counts for each pixel, and no variance lies within 1e-3 (relative) of
the threshold: the GPU's colours differ from the oracle's by ~1e-16 (libm), which
cannot flip a decision that far from the threshold.
"""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_stats  # noqa: E402

from test_trace_api import C_TO_CTYPES, C_TO_FIDDLE  # noqa: E402

CALLS = {
    "rtx_render_pixels_device": ["rtx_context*", "int32_t", "uint64_t", "const int32_t*", "double*", "double*",
                                 "int32_t*", "void*"],
    "rtx_render_pixels": ["rtx_context*", "int32_t", "uint64_t", "const int32_t*", "double*", "double*", "int32_t*"],
}


def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "rtx.h")).read()
    m = re.search(r"rtx_status\s+%s\(([^)]*)\);" % name, hdr)
    assert m, "include/rtx.h does not declare %s" % name
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    return [re.sub(r"\s*\w+$", "", a) for a in args]              # drop the parameter names


@pytest.mark.parametrize("name", sorted(CALLS))
def test_header_declares_the_call(name):
    assert _header_args(name) == CALLS[name]


def test_library_exports_them_and_refuses_a_null_context():
    from raytracing_rb_amd import _abi
    lib = _abi.load_library()
    assert hasattr(lib, "rtx_render_pixels_device") and hasattr(lib, "rtx_render_pixels")
    assert lib.rtx_render_pixels_device(None, 1, 1, None, None, None, None, None) == 6
    assert lib.rtx_render_pixels(None, 1, 1, None, None, None, None) == 6


@pytest.mark.parametrize("name", sorted(CALLS))
def test_ctypes_prototype_and_fiddle_extern_match_the_header(name):
    from raytracing_rb_amd import _abi, api, runtime
    args = _header_args(name)
    sig = {n: (r, a) for n, r, a in _abi.SIGNATURES}
    assert sig[name] == (C.c_int32, [C_TO_CTYPES[a] for a in args])
    rb = open(os.path.join(ROOT, "ext", "rtx", "lib", "rtx.rb")).read()
    assert "extern 'int %s(%s)'" % (name, ", ".join(C_TO_FIDDLE[a] for a in args)) in rb
    assert callable(runtime.Renderer.render_pixels) and callable(runtime.Renderer.render_pixels_device)
    assert callable(api.Camera.render_pixels) and callable(api.Camera.sampling)
    glue = open(os.path.join(ROOT, "ext", "rtx", "lib", "rtx", "reference.rb")).read()
    assert re.search(r"^\s*def render_pixels\(list\)", glue, flags=re.M)


def test_restatement_on_hand_made_samples():
    """Two samples a pixel, threshold 0.01: a flat pixel, one whose variance fires (max > pre and max <= pre),
    a raising pre sample, a raising extra sample."""
    c = np.zeros((4, 4, 3))
    c[0, :2] = [[0.25, 0.5, 0.125]] * 2                                # flat: variance 0
    c[1, :] = [[0.0, 0.0, 0.0], [1.0, 0.5, 0.25], [0.5, 0.5, 0.5], [0.25, 0.25, 0.25]]
    c[2, :] = c[1]
    c[3, :] = c[1]
    st = np.zeros((4, 4), np.int32)
    st[2, 1] = 3                                                       # a pre sample raises
    st[3, 3] = 2                                                       # an extra sample raises
    rgb, var, status, samples = pixel_stats.pixels(c, st, 0.01, 2, 4)
    assert rgb[0].tolist() == [0.25, 0.5, 0.125] and var[0] == 0.0 and samples[0] == 2
    # pixel 1: mean (0.5, 0.25, 0.125); max(c0 - mean) = -0.125, max(c1 - mean) = 0.5 -> (0.015625 + 0.25) / 2
    assert var[1] == 0.1328125 and samples[1] == 4 and status[1] == 0
    assert rgb[1].tolist() == [(0.5 * 2 + 0.75) / 4, (0.25 * 2 + 0.75) / 4, (0.125 * 2 + 0.75) / 4]
    assert status[2] == 3 and samples[2] == 2 and np.isnan(rgb[2]).all() and np.isnan(var[2])
    assert status[3] == 2 and samples[3] == 4 and np.isnan(rgb[3]).all() and var[3] == var[1]
    rgb, var, status, samples = pixel_stats.pixels(c[:, :2], st[:, :2], 0.01, 2, 1)       # max <= pre
    assert samples.tolist() == [2, 2, 2, 2] and rgb[1].tolist() == [1.0, 0.5, 0.25]      # (mean * 2 + 0) / 1
    mean, var2, fire = pixel_stats.expected(c[:, :2], st[:, :2], 0.01, 2, 4)
    assert fire.tolist() == [False, True, False, True] and mean[1].tolist() == [0.5, 0.25, 0.125]


@pytest.mark.parametrize("name", sorted(pixel_stats.CONFIGS))
def test_restated_decision_equals_the_oracles_sample_count(oracle_lib, name):
    from oracle.c_oracle import Oracle
    sd, cd = pixel_stats.load(name)
    pre, mx, thr = cd.pre_sample_times, cd.max_sample_times, cd.variant_threshold
    assert mx > pre
    oracle = Oracle(sd, cd)
    xy = pixel_stats.frame_xy(cd.width, cd.height)
    col, st, _ = pixel_stats.oracle_samples(oracle, xy)
    assert not st.any()                                               # no pixel of these frames raises
    rgb, var, status, samples = pixel_stats.pixels(col, st, thr, pre, mx)
    _, _, fire = pixel_stats.expected(col[:, :pre], st[:, :pre], thr, pre, mx)
    counts, ost = pixel_stats.oracle_counts(oracle, xy)
    assert not ost.any()
    assert np.array_equal(samples, counts), np.nonzero(samples != counts)[0][:5]
    assert np.array_equal(np.where(fire, mx, pre), counts)
    assert int(fire.sum()) == pixel_stats.EXTRAS[name], int(fire.sum())
    dist = np.abs(var - thr) / thr
    print(name, "extras %d of %d, least relative distance from the threshold %.3g" % (fire.sum(), len(xy), dist.min()))
    assert dist.min() >= 1e-3
    # and the restated colour is the oracle's own render_at
    ref, _, rc = oracle.render_pixels(xy)
    assert rc == 0 and np.array_equal(rgb.view(np.uint64), ref.view(np.uint64))


def test_mix_with_its_own_threshold_takes_no_extras(oracle_lib):
    """The list in which no pixel takes extra samples (tests/test_gpu_pixels.py): the mix frame under its own
    variant_threshold."""
    from conftest import scene_paths
    from oracle.c_oracle import Oracle
    from raytracing_rb_amd import config
    sd, cd = config.load_scene(*scene_paths("mix"), camera_overrides=dict(width=pixel_stats.W, height=pixel_stats.H))
    oracle = Oracle(sd, cd)
    xy = pixel_stats.frame_xy(cd.width, cd.height)
    col, st, _ = pixel_stats.oracle_samples(oracle, xy)
    _, var, fire = pixel_stats.expected(col[:, :cd.pre_sample_times], st[:, :cd.pre_sample_times],
                                        cd.variant_threshold, cd.pre_sample_times, cd.max_sample_times)
    assert not st.any() and not fire.any()
    assert (np.abs(var - cd.variant_threshold) / cd.variant_threshold).min() >= 1e-3
