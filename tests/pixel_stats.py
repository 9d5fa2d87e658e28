"""Camera#render_at's per-pixel arithmetic (camera.rb:70-99) restated in numpy
float64, operation for operation, over per-sample colours and statuses: what
rtx_render_pixels must give once the samples are traced.

    avg = (0 + c_0 + c_1 + ...) / pre                      camera.rb:74-79
    variance = sum_j max(c_j - avg) ** 2 / pre             :80-85  (.max of the vector, squared)
    if variance >= variant_threshold:                      :86
        avg = (avg * pre + (0 + c_pre + ...)) / max        :87-96  (max <= pre: no extra sample, + 0)

Every step is one elementwise binary64 operation over the pixels, so the bits
are those of a scalar loop in the same order (numpy contracts nothing).  A
sample's status is the rtx_status of its tree's first raise; the first raising
sample in render_at's order ends the pixel.
"""

import numpy as np

RTX_CNT_PRIMARY = 10           # include/rtx.h rtx_counter: lens_func samples


def _sum(c):
    """(0, 0, 0) + c[:, 0] + c[:, 1] + ... in sample order; c [n, k, 3]."""
    s = np.zeros((c.shape[0], 3), np.float64)
    for j in range(c.shape[1]):
        s = s + c[:, j]
    return s


def expected(colours, status, threshold, pre, max_samples):
    """colours [n, pre, 3], status [n, pre] of the pre samples -> (mean [n, 3],
    variance [n], fire bool [n]): the pre mean, the variance compared with the
    threshold and whether the test fires.  A pixel with a raising pre sample has
    NaN mean and variance and does not fire."""
    colours = np.asarray(colours, np.float64).reshape(-1, pre, 3)
    status = np.asarray(status, np.int32).reshape(-1, pre)
    with np.errstate(invalid="ignore"):
        avg = _sum(colours) / np.float64(pre)
        var = np.zeros(len(colours), np.float64)
        for j in range(pre):
            dd = colours[:, j] - avg
            mx = dd[:, 0].copy()
            mx = np.where(dd[:, 1] > mx, dd[:, 1], mx)
            mx = np.where(dd[:, 2] > mx, dd[:, 2], mx)
            var = var + mx * mx
        var = var / np.float64(pre)
        fire = var >= threshold
    bad = status.any(axis=1)
    avg[bad] = np.nan
    var[bad] = np.nan
    fire[bad] = False
    return avg, var, fire


def pixels(colours, status, threshold, pre, max_samples):
    """colours [n, ms, 3], status [n, ms] of all ms = max(pre, max) samples (the
    extra ones are read only where render_at takes them) -> (rgb [n, 3], variance
    [n], status [n], samples [n]) as rtx_render_pixels defines them."""
    ms = max(pre, max_samples)
    colours = np.asarray(colours, np.float64).reshape(-1, ms, 3)
    status = np.asarray(status, np.int32).reshape(-1, ms)
    n = len(colours)
    avg, var, fire = expected(colours[:, :pre], status[:, :pre], threshold, pre, max_samples)
    rgb = avg.copy()
    st = np.zeros(n, np.int32)
    samples = np.full(n, pre, np.int32)
    pre_bad = status[:, :pre] != 0
    for i in np.nonzero(pre_bad.any(axis=1))[0]:
        j = int(np.argmax(pre_bad[i]))
        st[i], samples[i] = status[i, j], j + 1
    if max_samples > pre:
        cv = _sum(colours[:, pre:max_samples])
        with np.errstate(invalid="ignore"):
            fin = (avg * np.float64(pre) + cv) / np.float64(max_samples)
        rgb[fire] = fin[fire]
        samples[fire] = max_samples
        ex_bad = status[:, pre:max_samples] != 0
        for i in np.nonzero(fire & ex_bad.any(axis=1))[0]:
            j = int(np.argmax(ex_bad[i]))
            st[i], samples[i] = status[i, pre + j], pre + j + 1
            rgb[i] = np.nan
    else:
        fin = (avg * np.float64(pre) + np.zeros(3)) / np.float64(max_samples)
        rgb[fire] = fin[fire]
    return rgb, var, st, samples


def frame_xy(width, height):
    """The frame's pixels row-major as int32 [n, 2] = (x, y)."""
    ys, xs = np.mgrid[0:height, 0:width]
    return np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], axis=1), np.int32)


def oracle_samples(oracle, xy, seed=1):
    """The oracle's side: Oracle.lens(x, y, j) -> Oracle.trace with the key (x, y, j) for every sample
    j < max(pre, max) of the pixels xy -> (colours [n, ms, 3], status [n, ms], rays [n, ms, 6])."""
    cam = oracle.camera
    ms = max(cam.pre_sample_times, cam.max_sample_times)
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    rays = np.array([[oracle.lens(int(x), int(y), j, seed) for j in range(ms)] for x, y in xy], np.float64)
    keys = np.array([[(x, y, j) for j in range(ms)] for x, y in xy], np.int32)
    col, st, _ = oracle.trace(rays.reshape(-1, 6), keys.reshape(-1, 3), seed)
    return col.reshape(-1, ms, 3), st.reshape(-1, ms), rays


def oracle_counts(oracle, xy, seed=1):
    """The oracle's own lens_func calls per pixel: Oracle.render_pixels(counts=True)[RTX_CNT_PRIMARY], one
    pixel a call -> (counts int64 [n], status int32 [n])."""
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    cnt = np.zeros(len(xy), np.int64)
    st = np.zeros(len(xy), np.int32)
    for i, p in enumerate(xy):
        _, s, _, c = oracle.render_pixels(p[None, :], seed=seed, counts=True)
        cnt[i], st[i] = int(c[RTX_CNT_PRIMARY]), s[0]
    return cnt, st


def gpu_samples(r, seed=1):
    """The GPU's own per-sample colours of the renderer's frame, row-major: Renderer.lens_rays(sample=j) ->
    Renderer.trace(check=False) with the keys (x, y, j) -> (colours [n, ms, 3], status [n, ms])."""
    ms = max(r.camera.pre_sample_times, r.camera.max_sample_times)
    xy = frame_xy(r.width, r.height)
    rays = np.stack([r.lens_rays(seed=seed, sample=j).reshape(-1, 6) for j in range(ms)], axis=1)
    keys = np.stack([np.concatenate([xy, np.full((len(xy), 1), j, np.int32)], axis=1) for j in range(ms)], axis=1)
    col, st = r.trace(np.ascontiguousarray(rays.reshape(-1, 6)), np.ascontiguousarray(keys.reshape(-1, 3), np.int32),
                      seed=seed, check=False)
    return col.reshape(-1, ms, 3), st.reshape(-1, ms)


# The three configurations of the parity checks: whole 24 x 14 frames.
W, H = 24, 14
CONFIGS = {
    "mix": ("mix", dict(variant_threshold=1e-6)),                           # pre 2, max 6
    "c2": ("c2", dict(pre_sample_times=3, max_sample_times=5)),
    "c0_default": ("c0_default", {}),                                       # pre 3, max 10
}
EXTRAS = {"mix": 135, "c2": 24, "c0_default": 22}      # pixels of the frame that take extra samples


def load(name, **more):
    """(scene descriptor, camera descriptor) of configuration `name` at W x H."""
    from conftest import scene_paths
    from raytracing_rb_amd import config
    scene, ov = CONFIGS[name]
    return config.load_scene(*scene_paths(scene), camera_overrides=dict(ov, width=W, height=H, **more))
