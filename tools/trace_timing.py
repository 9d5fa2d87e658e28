#!/usr/bin/env python3
"""Time rtx_trace_device under "trace_engine" 0 (lanes) and 1 (bounce levels) (GPU box;
DESIGN.md §3.22, profiles/trace/trace_timing.json).

    python tools/trace_timing.py [--out FILE.json] [--size 1024] [--warmup 3] [--reps 20]

Throughput: the lens rays of sample 0 of C2 (scenes/c2_camera.yml) and C4
(scenes/c4_camera.yml) at size x size, each scene's own trace_depth, in row-major
order and in one fixed random permutation (neighbouring lanes are then no
neighbouring pixels: what ray binning and the light buffer are worth then).
Crossover: n = 4^k, 2^6 .. size^2, of C2's row-major rays, every (size^2 / n)-th
one, so that each batch covers the whole frame (the first n would be sky);
the smallest n whose levels median is at or below the lanes median is the
threshold of "trace_engine" -1 (RTX_TRACE_LEVELS_MIN_RAYS, rtx_capi.cpp).
HIP events on the launch stream around each call, with a status buffer.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rt_map_timing import timed  # noqa: E402


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
    scenes = {"c2": (os.path.join(ROOT, "scenes", "c2_world.yml"), os.path.join(ROOT, "scenes", "c2_camera.yml")),
              "c4": (make_scenes.ensure_c4(), os.path.join(ROOT, "scenes", "c4_camera.yml"))}
    n = a.size * a.size
    res = {"rays": n, "launches": "%d warm-up + %d timed, HIP events, median (min-max)" % (a.warmup, a.reps),
           "throughput": {}, "crossover_c2": []}
    keys = np.empty((n, 3), np.int32)
    keys[:, 0] = np.tile(np.arange(a.size), a.size)
    keys[:, 1] = np.repeat(np.arange(a.size), a.size)
    keys[:, 2] = 0
    perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)
    for name, (world, camera) in scenes.items():
        sd, cd = config.load_scene(world, camera, camera_overrides=dict(width=a.size, height=a.size))
        r = Renderer(sd, cd)
        rays = torch.empty((n, 6), dtype=torch.float64, device=dev)
        r.lens_rays_device(rays.data_ptr(), stream=s.cuda_stream)
        d_keys = torch.from_numpy(keys).to(dev)
        rgb = torch.empty((n, 3), dtype=torch.float64, device=dev)
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        row = res["throughput"][name] = {"trace_depth": cd.trace_depth}
        first = {}
        for order, (R, K) in (("row_major", (rays, d_keys)),
                              ("permuted", (rays[perm].contiguous(), d_keys[perm].contiguous()))):
            for engine in (0, 1):
                r.set_option("trace_engine", engine)
                t = timed(lambda: r.trace_device(R, K, rgb, status, stream=s.cuda_stream), s, a.warmup, a.reps)
                assert r.get_option("trace_engine_last") == engine
                t["Mrays_per_s"] = n / t["median_ms"] / 1e3
                if engine == 1:
                    t["level_stats"] = r.level_stats()
                out = (rgb.clone(), status.clone())
                if order == "permuted":                          # the same rays: the same results, by ray
                    back = torch.empty_like(perm)
                    back[perm] = torch.arange(n, device=dev)
                    out = (out[0][back], out[1][back])
                ref = first.setdefault("ref", out)
                t["same_bits_as_first"] = bool(torch.equal(ref[0].view(torch.int64), out[0].view(torch.int64)) and
                                               torch.equal(ref[1], out[1]))
                row["%s_engine%d" % (order, engine)] = t
                print(name, order, engine, json.dumps(t), flush=True)
        if name == "c2":
            m = 64
            while m <= n:
                e = {"n": m}
                pick = torch.arange(m, device=dev) * (n // m)
                Rm, Km = rays[pick].contiguous(), d_keys[pick].contiguous()
                for engine in (0, 1):
                    r.set_option("trace_engine", engine)
                    e["engine%d" % engine] = timed(
                        lambda: r.trace_device(Rm, Km, rgb[:m], status[:m], stream=s.cuda_stream), s,
                        a.warmup, a.reps)
                e["levels_at_or_below_lanes"] = e["engine1"]["median_ms"] <= e["engine0"]["median_ms"]
                res["crossover_c2"].append(e)
                print("crossover", json.dumps(e), flush=True)
                m *= 4
            wins = [e["n"] for e in res["crossover_c2"] if e["levels_at_or_below_lanes"]]
            res["threshold"] = min(wins) if wins else "never"
        r.sync(s.cuda_stream)
        r.close()
    print("threshold", res.get("threshold"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
