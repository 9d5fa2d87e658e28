#!/usr/bin/env python3
"""Time rtx_rt_map_device against rtx_intersect_device + rtx_lit_area_device (GPU box;
DESIGN.md §3.21, profiles/rt_map/rt_map_timing.json).

    python tools/rt_map_timing.py [--out FILE.json] [--size 1024] [--warmup 3] [--reps 20]

Per scene (C2, C4; scenes/c2_camera.yml at size x size) and option set (default,
"bvh" 0): the level-0 items are rtx_lens_rays of sample 0, 2^20 at the default
size; HIP events on the launch stream around each device call, all output
buffers.  The two queries run in the same process on the same rays and on their
hits' intersection + delta (repeated to the item count where some rays miss), as
profiles/queries/queries_timing.json was measured.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, stream, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import make_scenes
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream()
    worlds = {"c2": os.path.join(ROOT, "scenes", "c2_world.yml"), "c4": make_scenes.ensure_c4()}
    n = a.size * a.size
    res = {"items": n, "launches": "%d warm-up + %d timed, HIP events, median (min-max)" % (a.warmup, a.reps), "scenes": {}}
    for name, world in worlds.items():
        sd, cd = config.load_scene(world, os.path.join(ROOT, "scenes", "c2_camera.yml"),
                                   camera_overrides=dict(width=a.size, height=a.size))
        cmax, L = 2 + cd.monte_carlo_diffusion_times, max(sd.desc.n_lights, 1)
        res["scenes"][name] = {"n_lights": sd.desc.n_lights, "trace_depth": cd.trace_depth}
        for label, opts in (("default", {}), ("bvh0", {"bvh": 0})):
            r = Renderer(sd, cd)
            for k, v in opts.items():
                r.set_option(k, v)
            rays = torch.empty((n, 6), dtype=torch.float64, device=dev)
            r.lens_rays_device(rays.data_ptr(), stream=s.cuda_stream)
            keys = np.empty((n, 4), np.int32)
            keys[:, 0] = np.tile(np.arange(a.size), a.size)
            keys[:, 1] = np.repeat(np.arange(a.size), a.size)
            keys[:, 2], keys[:, 3] = 0, cd.trace_depth
            d_keys = torch.from_numpy(keys).to(dev)
            info = torch.empty((n, 6), dtype=torch.int32, device=dev)
            ch = torch.empty((n, cmax, 9), dtype=torch.float64, device=dev)
            cp = torch.empty((n, cmax), dtype=torch.int64, device=dev)
            lf = torch.empty((n, L, 3), dtype=torch.float64, device=dev)
            ids = torch.empty((n, 3), dtype=torch.int32, device=dev)
            geom = torch.empty((n, 13), dtype=torch.float64, device=dev)

            def rt_map():
                r.rt_map_device(n, rays.data_ptr(), None, d_keys.data_ptr(), None, info.data_ptr(), ch.data_ptr(),
                                cp.data_ptr(), lf.data_ptr(), stream=s.cuda_stream)

            def intersect():
                r.intersect_device(n, rays.data_ptr(), ids.data_ptr(), geom.data_ptr(), stream=s.cuda_stream)
            t_map = timed(rt_map, s, a.warmup, a.reps)
            t_int = timed(intersect, s, a.warmup, a.reps)
            hit = ids[:, 0] >= 0
            T = (geom[hit, 1:4] + geom[hit, 10:13]).contiguous()
            hits = int(T.shape[0])
            T = T.repeat((n + hits - 1) // hits, 1)[:n].contiguous()
            area = torch.empty((n, L), dtype=torch.float64, device=dev)
            color = torch.empty((n, L, 3), dtype=torch.float64, device=dev)
            status = torch.empty((n,), dtype=torch.int32, device=dev)

            def lit_area():
                r.lit_area_device(n, T.data_ptr(), None, area.data_ptr(), color.data_ptr(), status.data_ptr(),
                                  stream=s.cuda_stream)
            t_lit = timed(lit_area, s, a.warmup, a.reps)
            kinds = torch.bincount(info[:, 1] + 1, minlength=6).cpu().tolist()
            res["scenes"][name][label] = {
                "hits": hits, "kinds_-1_to_4": kinds, "children": int(info[:, 3].sum().item()),
                "rt_map": t_map, "intersect": t_int, "lit_area": t_lit,
                "intersect_plus_lit_area_median_ms": t_int["median_ms"] + t_lit["median_ms"]}
            print(name, label, json.dumps(res["scenes"][name][label]), flush=True)
            r.sync(s.cuda_stream)
            r.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
