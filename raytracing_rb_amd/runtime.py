"""Thin Python handle over librtx (``include/rtx.h``).

``Renderer`` owns one ``rtx_context`` (one HIP device) with an uploaded scene
and camera.  Host-buffer calls are synchronous; ``*_device`` calls take raw
device pointers (e.g. ``torch.Tensor.data_ptr()``) and a HIP stream handle and
return immediately.  Errors raise ``RtxError`` carrying the reference's raise
site (``rtx_status``).  There is no CPU fallback: without librtx.so nothing here
works.
"""

import ctypes as C

import numpy as np

from . import _abi
from ._abi import RTX_NCOUNT, COUNTER_NAMES, load_library


class RtxError(RuntimeError):
    KINDS = {1: "zero_vec", 2: "color_gt1", 3: "domain", 4: "hip", 5: "rccl", 6: "invalid", 7: "nomem",
             8: "type"}

    def __init__(self, status, msg):
        super().__init__("%s (rtx_status %d)" % (msg, status))
        self.status = status
        self.kind = self.KINDS.get(status, "unknown")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Renderer:
    def __init__(self, scene, camera, device=0):
        """scene: config.SceneDescriptor; camera: _abi.CameraDesc."""
        self.lib = load_library()
        self.h = C.c_void_p()
        st = self.lib.rtx_context_create(device, C.byref(self.h))
        if st:
            raise RtxError(st, "rtx_context_create failed")
        self.device = device
        self._scene = scene
        self.camera = camera
        self._check(self.lib.rtx_scene_upload(self.h, C.byref(scene.desc)))
        self._check(self.lib.rtx_camera_set(self.h, C.byref(camera)))

    # ------------------------------------------------------------ plumbing
    def _check(self, st):
        if st:
            raise RtxError(st, self.lib.rtx_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.rtx_context_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def width(self):
        return self.camera.width

    @property
    def height(self):
        return self.camera.height

    def set_camera(self, camera):
        self.camera = camera
        self._check(self.lib.rtx_camera_set(self.h, C.byref(camera)))

    def set_option(self, key, value):
        self._check(self.lib.rtx_set_option(self.h, key.encode(), int(value)))

    # ------------------------------------------------------------ host API
    def render(self, x0=0, y0=0, x1=None, y1=None, seed=1):
        """Float64 framebuffer [y1-y0, x1-x0, 3] (row = y, top first)."""
        x1 = self.width if x1 is None else x1
        y1 = self.height if y1 is None else y1
        out = np.empty((y1 - y0, x1 - x0, 3), np.float64)
        self._check(self.lib.rtx_render(self.h, x0, y0, x1, y1, seed, _dp(out), (x1 - x0) * 3))
        return out

    def render_at(self, x, y, seed=1):
        out = np.empty(3, np.float64)
        self._check(self.lib.rtx_render_at(self.h, x, y, seed, _dp(out)))
        return out

    def render_pixels(self, xy, seed=1, check=True):
        """Camera#render_at for the pixels xy int32 [n, 2] = (x, y) in one call
        (rtx_render_pixels): colours [n, 3] with the bits render() gives those
        pixels.  Any int32 coordinates; duplicates are independent entries.
        check=True raises RtxError for the first raising pixel by index.
        check=False returns (rgb, variance [n], status int32 [n], samples int32
        [n]): the variance render_at compares with variant_threshold, every
        pixel's own rtx_status and the lens_func calls render_at made for it; a
        raising pixel's colour is NaN (its variance too if a pre sample raised)."""
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        n = len(xy)
        rgb = np.empty((n, 3), np.float64)
        var = np.empty(n, np.float64)
        info = np.zeros((n, 2), np.int32)
        st = self.lib.rtx_render_pixels(self.h, n, seed, C.c_void_p(xy.ctypes.data), C.c_void_p(rgb.ctypes.data),
                                        C.c_void_p(var.ctypes.data), C.c_void_p(info.ctypes.data))
        if st and (check or not info[:, 0].any()):   # (a status without a raising pixel: an argument or HIP error)
            self._check(st)
        return rgb if check else (rgb, var, info[:, 0].copy(), info[:, 1].copy())

    def trace(self, rays, keys, seed=1, check=True):
        """RayTracer#trace_sync for rays [n, 6] = (front, position) with the RNG keys
        [n, 3] = (x, y, sample) (rtx_trace) -> colours [n, 3].  check=True raises
        RtxError for the first raising ray.  check=False returns (colours, status
        int32 [n]): every ray's own rtx_status, a raising ray's colour NaN, through
        rtx_trace_device (option "trace_engine"; its default -1 runs the bounce
        levels here, as 1)."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        if len(keys) != len(rays):
            raise ValueError("one key per ray")
        if not check:
            return self._trace_statuses(rays, keys, seed)
        out = np.empty((len(rays), 3), np.float64)
        self._check(self.lib.rtx_trace(self.h, len(rays), _dp(rays),
                                       keys.ctypes.data_as(C.POINTER(C.c_int32)), seed, _dp(out)))
        return out

    def _trace_statuses(self, rays, keys, seed):
        import torch
        dev = torch.device("cuda", self.device)
        n = len(rays)
        d_rays, d_keys = torch.tensor(rays, device=dev), torch.tensor(keys, device=dev)   # (copies: read-only arrays too)
        d_rgb = torch.empty((n, 3), dtype=torch.float64, device=dev)
        d_status = torch.zeros(n, dtype=torch.int32, device=dev)
        engine = self.get_option("trace_engine")
        if engine == -1:
            self.set_option("trace_engine", 1)
        try:
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream().cuda_stream
                self.trace_device(d_rays, d_keys, d_rgb, d_status, seed=seed, stream=stream)
                return d_rgb.cpu().numpy(), d_status.cpu().numpy()
        finally:
            if engine == -1:
                self.set_option("trace_engine", -1)

    def path_trace(self, rays):
        """RayTracer#path_trace_sync for rays [n, 6] = (front, position) -> [n, 3]."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        out = np.empty((len(rays), 3), np.float64)
        self._check(self.lib.rtx_path_trace(self.h, len(rays), _dp(rays), _dp(out)))
        return out

    def first_hit(self, x0=0, y0=0, x1=None, y1=None, seed=1, sample=0):
        """First-hit feature buffers of camera sample ``sample`` (rtx_first_hit):
        lens_func(x, y, sample) -> World#intersect per pixel, no shading.  A dict of
        arrays over the region [H, W] (row = y, top first): ``object`` (index into
        world_objects, -1 = miss), ``direction`` (0 :in, 1 :out), ``data`` (box face
        or -1), int32; ``depth`` [H, W] (max_distance on a miss); ``position``,
        ``normal`` (normalized), ``albedo`` [H, W, 3], float64."""
        x1 = self.width if x1 is None else x1
        y1 = self.height if y1 is None else y1
        h, w = max(y1 - y0, 0), max(x1 - x0, 0)
        ids = np.empty((h, w, 3), np.int32)
        geom = np.empty((h, w, 10), np.float64)
        self._check(self.lib.rtx_first_hit(self.h, x0, y0, x1, y1, seed, sample,
                                           ids.ctypes.data_as(C.POINTER(C.c_int32)), _dp(geom)))
        return split_first_hit(ids, geom)

    def intersect(self, rays):
        """World#intersect for rays [n, 6] = (front, position) (rtx_intersect): the
        dict of ``first_hit`` over [n] (``depth`` = ray.distance(intersection)) plus
        ``delta`` [n, 3], the offset local_lights is called with (intersection + delta)."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        n = len(rays)
        ids = np.empty((n, 3), np.int32)
        geom = np.empty((n, 13), np.float64)
        self._check(self.lib.rtx_intersect(self.h, n, _dp(rays), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                           _dp(geom)))
        return split_intersect(ids, geom)

    def lit_area(self, targets, lights=None, want_color=True, check=True):
        """World#lit_area / #local_lights for targets [n, 3] (rtx_lit_area) ->
        (area [n, L], color [n, L, 3] or None, status int32 [n]).  lights None: the
        scene's lights in order (L = their number); else [n, 4] = one explicit
        {position, radius} per target (L = 1, no colour).  status[i] is the rtx_status
        of target i's first raise in light order (3: cover_area's Math.acos), its
        entries from that light on NaN.  check=True raises RtxError for the first
        raising target; check=False returns the statuses."""
        targets = np.ascontiguousarray(targets, np.float64).reshape(-1, 3)
        n = len(targets)
        if lights is not None:
            lights = np.ascontiguousarray(lights, np.float64).reshape(-1, 4)
            if len(lights) != n:
                raise ValueError("one explicit light per target")
            want_color = False
        nl = 1 if lights is not None else self._scene.desc.n_lights
        area = np.empty((n, nl), np.float64)
        color = np.empty((n, nl, 3), np.float64) if want_color else None
        status = np.zeros(n, np.int32)
        st = self.lib.rtx_lit_area(self.h, n, _dp(targets), _dp(lights) if lights is not None else None, _dp(area),
                                   _dp(color) if want_color else None, status.ctypes.data_as(C.POINTER(C.c_int32)))
        if st and (check or not status.any()):      # (a status without a raising target: an argument or HIP error)
            self._check(st)
        return area, color, status

    def lens_rays(self, x0=0, y0=0, x1=None, y1=None, seed=1, sample=0):
        """Camera#lens_func(x, y, sample) for the region (rtx_lens_rays): float64
        [H, W, 6] = (front, position), row = y, top first: the rays a render of the
        same seed traces for that sample."""
        x1 = self.width if x1 is None else x1
        y1 = self.height if y1 is None else y1
        rays = np.empty((max(y1 - y0, 0), max(x1 - x0, 0), 6), np.float64)
        self._check(self.lib.rtx_lens_rays(self.h, x0, y0, x1, y1, seed, sample, _dp(rays)))
        return rays

    def rt_map(self, rays, keys, att=None, paths=None, seed=1, check=True, children=True, child_paths=True,
               leaves=True):
        """RayTracer#rt_map, one call per item (rtx_rt_map).  rays [n, 6] = (front,
        position); keys int32 [n, 4] = (x, y, sample, remaining trace_depth); att
        [n, 3] or None (ones); paths uint64 [n] or None (roots).  A dict of arrays:
        ``status``, ``kind`` (0 dead, 1 highlight, 2 miss, 3 lit hit, 4 unlit hit,
        -1 a raise), ``object``, ``n_children``, ``n_leaves``, ``direction`` int32
        [n]; ``children`` [n, CMAX, 9] = (front, position, attenuation),
        ``child_paths`` uint64 [n, CMAX], ``leaves`` [n, LMAX, 3], with CMAX = 2 +
        monte_carlo_diffusion_times and LMAX = max(lights, 1); an output switched
        off by its flag is None.  check=True raises RtxError for the first raising
        item; check=False returns the statuses."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        n = len(rays)
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 4)
        if len(keys) != n:
            raise ValueError("one key per ray")
        u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
        if att is not None:
            att = np.ascontiguousarray(att, np.float64).reshape(-1, 3)
            if len(att) != n:
                raise ValueError("one attenuation per ray")
        if paths is not None:
            paths = np.ascontiguousarray(paths, np.uint64).reshape(-1)
            if len(paths) != n:
                raise ValueError("one path per ray")
        cmax = 2 + self.camera.monte_carlo_diffusion_times
        lmax = max(self._scene.desc.n_lights, 1)
        info = np.zeros((n, 6), np.int32)
        ch = np.empty((n, cmax, 9), np.float64) if children else None
        cp = np.empty((n, cmax), np.uint64) if child_paths else None
        lf = np.empty((n, lmax, 3), np.float64) if leaves else None
        st = self.lib.rtx_rt_map(self.h, n, seed, _dp(rays), _dp(att) if att is not None else None,
                                 keys.ctypes.data_as(i32p), paths.ctypes.data_as(u64p) if paths is not None else None,
                                 info.ctypes.data_as(i32p), _dp(ch) if children else None,
                                 cp.ctypes.data_as(u64p) if child_paths else None, _dp(lf) if leaves else None)
        if st and (check or not info[:, 0].any()):   # (a status without a raising item: an argument or HIP error)
            self._check(st)
        out = split_rt_map(info)
        out.update(children=ch, child_paths=cp, leaves=lf)
        return out

    def count_work(self, seed=1):
        cnt = (C.c_uint64 * RTX_NCOUNT)()
        self._check(self.lib.rtx_count_work(self.h, seed, cnt))
        return dict(zip(COUNTER_NAMES, [int(v) for v in cnt]))

    # ------------------------------------------------------------ device API
    def render_device(self, d_out, seed=1, x0=0, y0=0, x1=None, y1=None, row_stride=None, stream=None):
        x1 = self.width if x1 is None else x1
        y1 = self.height if y1 is None else y1
        row_stride = (x1 - x0) * 3 if row_stride is None else row_stride
        self._check(self.lib.rtx_render_device(self.h, x0, y0, x1, y1, seed, C.c_void_p(d_out), row_stride,
                                               C.c_void_p(stream or 0)))

    def first_hit_device(self, d_ids, d_geom, seed=1, sample=0, x0=0, y0=0, x1=None, y1=None, stream=None):
        """rtx_first_hit_device: d_ids int32 [rows, cols, 3], d_geom float64 [rows, cols, 10]
        (device pointers; either may be None).  Records no raise."""
        x1 = self.width if x1 is None else x1
        y1 = self.height if y1 is None else y1
        self._check(self.lib.rtx_first_hit_device(self.h, x0, y0, x1, y1, seed, sample, C.c_void_p(d_ids or 0),
                                                  C.c_void_p(d_geom or 0), C.c_void_p(stream or 0)))

    def intersect_device(self, n, d_rays, d_ids, d_geom, stream=None):
        """rtx_intersect_device: d_rays float64 [n, 6], d_ids int32 [n, 3], d_geom float64
        [n, 13] (device pointers; one of the outputs may be None).  Records no raise."""
        self._check(self.lib.rtx_intersect_device(self.h, n, C.c_void_p(d_rays or 0), C.c_void_p(d_ids or 0),
                                                  C.c_void_p(d_geom or 0), C.c_void_p(stream or 0)))

    def lit_area_device(self, n, d_targets, d_lights, d_area, d_color=None, d_status=None, stream=None):
        """rtx_lit_area_device: d_targets float64 [n, 3], d_lights None or float64 [n, 4],
        d_area float64 [n, L], d_color None or float64 [n, L, 3], d_status None or int32 [n]
        (device pointers).  Raises go to d_status only."""
        self._check(self.lib.rtx_lit_area_device(self.h, n, C.c_void_p(d_targets or 0), C.c_void_p(d_lights or 0),
                                                 C.c_void_p(d_area or 0), C.c_void_p(d_color or 0),
                                                 C.c_void_p(d_status or 0), C.c_void_p(stream or 0)))

    def lens_rays_device(self, d_rays, seed=1, sample=0, x0=0, y0=0, x1=None, y1=None, stream=None):
        """rtx_lens_rays_device: d_rays float64 [rows, cols, 6] (device pointer)."""
        x1 = self.width if x1 is None else x1
        y1 = self.height if y1 is None else y1
        self._check(self.lib.rtx_lens_rays_device(self.h, x0, y0, x1, y1, seed, sample, C.c_void_p(d_rays or 0),
                                                  C.c_void_p(stream or 0)))

    def rt_map_device(self, n, d_rays, d_att, d_keys, d_paths, d_info, d_children=None, d_child_paths=None,
                      d_leaves=None, seed=1, stream=None):
        """rtx_rt_map_device: d_rays float64 [n, 6], d_att None or float64 [n, 3], d_keys
        int32 [n, 4], d_paths None or uint64 [n], d_info int32 [n, 6], and, each or None,
        d_children float64 [n, CMAX, 9], d_child_paths uint64 [n, CMAX], d_leaves float64
        [n, LMAX, 3] (device pointers).  Raises go to d_info only."""
        self._check(self.lib.rtx_rt_map_device(self.h, n, seed, C.c_void_p(d_rays or 0), C.c_void_p(d_att or 0),
                                               C.c_void_p(d_keys or 0), C.c_void_p(d_paths or 0),
                                               C.c_void_p(d_info or 0), C.c_void_p(d_children or 0),
                                               C.c_void_p(d_child_paths or 0), C.c_void_p(d_leaves or 0),
                                               C.c_void_p(stream or 0)))

    def trace_device(self, d_rays, d_keys, d_rgb, d_status=None, seed=1, stream=None, n=None):
        """rtx_trace_device: d_rays float64 [n, 6], d_keys int32 [n, 3], d_rgb float64
        [n, 3], d_status None or int32 [n]: torch tensors on this renderer's device
        (n = rows of d_rays) or raw device pointers with n given.  Asynchronous on
        `stream`; raises go to d_status only, a raising ray's colour is NaN."""
        def ptr(t):
            return 0 if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        if n is None:
            if not hasattr(d_rays, "numel"):
                raise ValueError("raw device pointers need n")
            n = d_rays.numel() // 6
            for t, per in ((d_keys, 3), (d_rgb, 3), (d_status, 1)):
                if t is not None and hasattr(t, "numel") and t.numel() < n * per:
                    raise ValueError("a buffer is smaller than the %d rays need" % n)
        self._check(self.lib.rtx_trace_device(self.h, n, seed, C.c_void_p(ptr(d_rays)), C.c_void_p(ptr(d_keys)),
                                              C.c_void_p(ptr(d_rgb)), C.c_void_p(ptr(d_status)),
                                              C.c_void_p(stream or 0)))

    def render_pixels_device(self, d_xy, d_rgb, d_variance=None, d_info=None, seed=1, stream=None, n=None):
        """rtx_render_pixels_device: d_xy int32 [n, 2], d_rgb float64 [n, 3], d_variance
        None or float64 [n], d_info None or int32 [n, 2] = (status, samples): torch
        tensors on this renderer's device (n = rows of d_xy) or raw device pointers
        with n given.  Asynchronous on `stream`; raises go to d_info only, a raising
        pixel's colour is NaN."""
        def ptr(t):
            return 0 if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else int(t))
        if n is None:
            if not hasattr(d_xy, "numel"):
                raise ValueError("raw device pointers need n")
            n = d_xy.numel() // 2
            for t, per in ((d_rgb, 3), (d_variance, 1), (d_info, 2)):
                if t is not None and hasattr(t, "numel") and t.numel() < n * per:
                    raise ValueError("a buffer is smaller than the %d pixels need" % n)
        self._check(self.lib.rtx_render_pixels_device(self.h, n, seed, C.c_void_p(ptr(d_xy)), C.c_void_p(ptr(d_rgb)),
                                                      C.c_void_p(ptr(d_variance)), C.c_void_p(ptr(d_info)),
                                                      C.c_void_p(stream or 0)))

    def rows_per_rank(self, tile_rows, nranks):
        return self.lib.rtx_tiles_rows_per_rank(self.height, tile_rows, nranks)

    def render_tiles_device(self, d_packed, tile_rows, rank, nranks, seed=1, stream=None):
        self._check(self.lib.rtx_render_tiles_device(self.h, tile_rows, rank, nranks, seed, C.c_void_p(d_packed),
                                                     C.c_void_p(stream or 0)))

    def render_tile_list_device(self, d_packed, tiles, tile_rows, seed=1, stream=None):
        """The tile_rows-row tiles `tiles` (image tile indices; past the bottom: padding)
        into packed rows k * tile_rows (rtx_render_tile_list_device)."""
        t = np.ascontiguousarray(tiles, np.int32)
        self._check(self.lib.rtx_render_tile_list_device(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), len(t),
                                                         tile_rows, seed, C.c_void_p(d_packed),
                                                         C.c_void_p(stream or 0)))

    def tile_probe(self):
        """Probe weights per 8x8 tile [ceil(H/8), ceil(W/8)] without rendering (rtx_tile_probe)."""
        tx, ty = (self.width + 7) // 8, (self.height + 7) // 8
        out = np.zeros(tx * ty, np.int64)
        self._check(self.lib.rtx_tile_probe(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), len(out)))
        return out.reshape(ty, tx)

    def tile_rays(self):
        """Rays per 8x8 tile [ceil(H/8), ceil(W/8)] of the last whole-frame level render (rtx_tile_rays)."""
        ty, tx = (self.height + 7) // 8, (self.width + 7) // 8
        out = np.zeros(ty * tx, np.int64)
        self._check(self.lib.rtx_tile_rays(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), len(out)))
        return out.reshape(ty, tx)

    def get_option(self, key):
        v = C.c_int64()
        self._check(self.lib.rtx_get_option(self.h, key.encode(), C.byref(v)))
        return v.value

    ENGINES = {0: "lanes", 1: "levels"}

    def engine(self):
        """Name of the ray-tree engine the next render of this scene and camera
        runs (read-only option "engine_effective": "engine", except that the
        bounce-level engine hands monte_carlo_diffusion_times > 14 to the lanes
        engine).  A camera whose ray stack, 1 +
        (trace_depth - 1) * (1 + monte_carlo_diffusion_times), exceeds 64 entries
        (every trace_depth > 64) is refused by both: RtxError, kind "invalid"."""
        return self.ENGINES[self.get_option("engine_effective")]

    def level_stats(self):
        """Bounce-level engine statistics of the last render call: {"redo", "dropped", "rays": [per level]}."""
        n = 2 + 65
        out = (C.c_int64 * n)()
        self._check(self.lib.rtx_level_stats(self.h, out, n))
        rays = list(out[2:])
        while rays and rays[-1] == 0:
            rays.pop()
        return {"redo": out[0], "dropped": out[1], "rays": rays}

    def kernel_time(self):
        """(total ms, launches) of the ray-tree kernel launches of the last render
        call (HIP events on the launch stream; needs set_option("kernel_events", 1))."""
        ms = C.c_double()
        n = C.c_int32()
        self._check(self.lib.rtx_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def sync(self, stream=None):
        self._check(self.lib.rtx_sync(self.h, C.c_void_p(stream or 0)))

    def quantize_device(self, d_rgb, d_rgba, png_gem_blend=True, stream=None, width=None, height=None):
        w = self.width if width is None else width
        h = self.height if height is None else height
        st = self.lib.rtx_quantize_device(C.c_void_p(d_rgb), w, h, w * 3, int(png_gem_blend), C.c_void_p(d_rgba),
                                          C.c_void_p(stream or 0))
        if st:
            raise RtxError(st, "rtx_quantize_device failed")


def split_first_hit(ids, geom):
    """The named views of rtx_first_hit's buffers: ids [H, W, 3], geom [H, W, 10]."""
    return {"object": ids[..., 0], "direction": ids[..., 1], "data": ids[..., 2], "depth": geom[..., 0],
            "position": geom[..., 1:4], "normal": geom[..., 4:7], "albedo": geom[..., 7:10]}


def split_intersect(ids, geom):
    """The named views of rtx_intersect's buffers: ids [n, 3], geom [n, 13]."""
    out = split_first_hit(ids, geom)
    out["delta"] = geom[..., 10:13]
    return out


def split_rt_map(info):
    """The named views of rtx_rt_map's info buffer [n, 6]."""
    return {"status": info[..., 0], "kind": info[..., 1], "object": info[..., 2], "n_children": info[..., 3],
            "n_leaves": info[..., 4], "direction": info[..., 5]}


def render_multi(renderers, tile_rows=8, seed=1):
    """Camera#render_fork over several contexts in one process (rtx_render_multi):
    renderer k renders rank k's tiles on its device, ONE RCCL gather to the first
    renderer's device.  Returns the float64 frame [H, W, 3]."""
    if not renderers:
        raise ValueError("no renderers")
    lib = load_library()
    r0 = renderers[0]
    hs = (C.c_void_p * len(renderers))(*[r.h.value for r in renderers])
    out = np.empty((r0.height, r0.width, 3), np.float64)
    st = lib.rtx_render_multi(hs, len(renderers), tile_rows, seed, _dp(out), r0.width * 3)
    if st:
        raise RtxError(st, lib.rtx_last_error(r0.h).decode())
    return out


def render_multi_plan(renderers, plan, tile_rows=8, seed=1):
    """render_multi with explicit tile lists (rtx_render_multi_plan): plan[k] is
    renderer k's list of tile_rows-row tiles (equal lengths, padded past the
    bottom, e.g. tiles.lpt_plan).  Returns the float64 frame [H, W, 3]."""
    if not renderers or len(plan) != len(renderers):
        raise ValueError("one tile list per renderer")
    lib = load_library()
    r0 = renderers[0]
    per = len(plan[0])
    flat = np.ascontiguousarray(np.asarray(plan, np.int32).reshape(-1))
    hs = (C.c_void_p * len(renderers))(*[r.h.value for r in renderers])
    out = np.empty((r0.height, r0.width, 3), np.float64)
    st = lib.rtx_render_multi_plan(hs, len(renderers), tile_rows, flat.ctypes.data_as(C.POINTER(C.c_int32)), per,
                                   seed, _dp(out), r0.width * 3)
    if st:
        raise RtxError(st, lib.rtx_last_error(r0.h).decode())
    return out


def lpt_plan_native(costs, nranks):
    """rtx_lpt_plan (host C++): the same plan as tiles.lpt_plan."""
    lib = load_library()
    c = np.ascontiguousarray(np.asarray(costs, np.int64))
    per = C.c_int32(0)
    st = lib.rtx_lpt_plan(c.ctypes.data_as(C.POINTER(C.c_int64)), len(c), nranks, None, 0, C.byref(per))
    if st:
        raise RtxError(st, "rtx_lpt_plan failed")
    out = np.zeros(nranks * per.value, np.int32)
    st = lib.rtx_lpt_plan(c.ctypes.data_as(C.POINTER(C.c_int64)), len(c), nranks,
                          out.ctypes.data_as(C.POINTER(C.c_int32)), per.value, C.byref(per))
    if st:
        raise RtxError(st, "rtx_lpt_plan failed")
    return [list(map(int, out[k * per.value:(k + 1) * per.value])) for k in range(nranks)]


def device_count():
    return load_library().rtx_device_count()


def quantize(rgb, png_gem_blend=True):
    """array_to_color + canvas point (camera.rb:105,153-156) on the GPU -> RGBA8 [H, W, 4]."""
    lib = load_library()
    rgb = np.ascontiguousarray(rgb, np.float64)
    h, w, _ = rgb.shape
    out = np.empty((h, w, 4), np.uint8)
    st = lib.rtx_quantize(_dp(rgb), w, h, w * 3, int(png_gem_blend), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if st:
        raise RtxError(st, "rtx_quantize failed")
    return out


def vec3_lib():
    return load_library()


__all__ = ["Renderer", "RtxError", "quantize", "render_multi", "render_multi_plan", "lpt_plan_native", "device_count",
           "_abi"]
