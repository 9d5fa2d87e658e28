#!/usr/bin/env python3
"""Time rtx_render_pixels (GPU box; DESIGN.md §3.23, profiles/pixels/pixels_timing.json).

    python tools/pixels_timing.py [--out FILE.json] [--width 1920] [--height 1080] [--warmup 3] [--reps 20]
                                  [--at-cap 1024]

scenes/c0_world.yml under scenes/camera.yml (pre 3, max 10) at width x height.

scattered   n = 64, 1,024 and 16,384 pixels, every (W H / n)-th of the frame: one rtx_render_pixels call
            against a loop of rtx_render_at over the same pixels, the loop capped at --at-cap calls
            (`at_calls`; `at_ms_per_pixel` is what scales).  Both are synchronous host calls, so a host clock
            around each; the two alternate within every repetition.
frame       the whole frame as a row-major list through rtx_render_pixels_device against
            rtx_render_device, HIP events around each call, alternating.
extras      the extras pass of the whole-frame list: the call under the scene's camera minus the call
            under the same camera with max_sample_times = pre_sample_times (the same pre pass and pixel
            stage, no extras pass), and the same difference with variant_threshold 0 (every pixel listed:
            the pass at its capacity, all of it live).  `live_fraction` is the listed pixels' share.
            These three are timed one after the other, each with its own warm-up, not alternating: their
            calls take from 2 to 17 GB from the stream-ordered pool, and alternating them makes the pool
            shrink and grow between calls (`alternating`, kept for the record, shows what that costs).
3 warm-up + 20 timed repetitions, median (min-max).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def alternate(fns, warmup, reps, clock):
    """Each repetition runs every variant once, in order; clock(fn) -> ms."""
    for _ in range(warmup):
        for fn in fns.values():
            clock(fn)
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(clock(fn))
    return {k: stats(v) for k, v in ts.items()}


def blocks(fns, warmup, reps, clock):
    """Each variant on its own: its warm-up, then its timed repetitions."""
    out = {}
    for k, fn in fns.items():
        for _ in range(warmup):
            clock(fn)
        out[k] = stats([clock(fn) for _ in range(reps)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--at-cap", type=int, default=1024)
    a = ap.parse_args()
    import torch
    from raytracing_rb_amd import config
    from raytracing_rb_amd.runtime import Renderer
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream()
    W, H = a.width, a.height
    world, camera = os.path.join(ROOT, "scenes", "c0_world.yml"), os.path.join(ROOT, "scenes", "camera.yml")

    def renderer(**ov):
        sd, cd = config.load_scene(world, camera, camera_overrides=dict(ov, width=W, height=H))
        return Renderer(sd, cd), cd

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    r, cd = renderer()
    pre, mx = cd.pre_sample_times, cd.max_sample_times
    res = {"frame_size": [W, H], "pre": pre, "max": mx,
           "repetitions": "%d warm-up + %d timed, the variants alternating, median (min-max)" % (a.warmup, a.reps),
           "scattered": [], "frame": {}, "extras": {}}
    ys, xs = np.mgrid[0:H, 0:W]
    frame_xy = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], axis=1), np.int32)

    for n in (64, 1024, 16384):
        xy = np.ascontiguousarray(frame_xy[np.arange(n) * (W * H // n)])
        calls = min(n, a.at_cap)
        sub = xy[np.arange(calls) * (n // calls)]              # the capped loop still covers the frame

        def loop():
            for x, y in sub:
                r.render_at(int(x), int(y))

        t = alternate({"pixels": lambda: r.render_pixels(xy), "render_at": loop}, a.warmup, a.reps, host_ms)
        one = r.render_pixels(sub)
        same = all(np.array_equal(one[k].view(np.uint64), r.render_at(int(x), int(y)).view(np.uint64))
                   for k, (x, y) in list(enumerate(sub))[:: max(1, calls // 16)])
        e = {"n": n, "pixels": t["pixels"], "at_calls": calls, "render_at_loop": t["render_at"],
             "at_ms_per_pixel": t["render_at"]["median_ms"] / calls,
             "pixels_ms_per_pixel": t["pixels"]["median_ms"] / n,
             "render_at_for_n_over_pixels": t["render_at"]["median_ms"] / calls * n / t["pixels"]["median_ms"],
             "same_bits_checked": bool(same), "trace_engine_last": r.get_option("trace_engine_last")}
        res["scattered"].append(e)
        print("scattered", json.dumps(e), flush=True)

    # the whole frame as a list against the rectangle render
    d_xy = torch.from_numpy(frame_xy).to(dev)
    npx = W * H
    rgb = torch.empty((npx, 3), dtype=torch.float64, device=dev)
    var = torch.empty((npx,), dtype=torch.float64, device=dev)
    info = torch.empty((npx, 2), dtype=torch.int32, device=dev)
    fb = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
    t = alternate({"pixels_device": lambda: r.render_pixels_device(d_xy, rgb, var, info, stream=s.cuda_stream),
                   "render_device": lambda: r.render_device(fb.data_ptr(), stream=s.cuda_stream)},
                  a.warmup, a.reps, event_ms)
    torch.cuda.synchronize()
    inf = info.cpu().numpy()
    res["frame"] = dict(t, pixels=npx, list_over_render=t["pixels_device"]["median_ms"] / t["render_device"]["median_ms"],
                        same_bits=bool(torch.equal(rgb.view(torch.int64), fb.view(-1, 3).view(torch.int64))),
                        samples=int(inf[:, 1].sum()), raising_pixels=int((inf[:, 0] != 0).sum()))
    r.set_option("trace_engine", 1)
    r.render_pixels_device(d_xy, rgb, var, info, stream=s.cuda_stream)
    res["frame"]["level_stats"] = r.level_stats()
    r.set_option("trace_engine", -1)
    print("frame", json.dumps(res["frame"]), flush=True)

    # the extras pass: at its capacity launch with the scene's live count, and all live
    r_none, _ = renderer(max_sample_times=pre)
    r_all, _ = renderer(variant_threshold=0.0)
    call = lambda q: (lambda: q.render_pixels_device(d_xy, rgb, var, info, stream=s.cuda_stream))   # noqa: E731
    variants = {"scene": call(r), "no_extras_pass": call(r_none), "all_extras": call(r_all)}
    t = blocks(variants, a.warmup, a.reps, event_ms)
    t["alternating"] = alternate(variants, 1, 5, event_ms)
    listed = int((inf[:, 1] > pre).sum())
    ex = t["scene"]["median_ms"] - t["no_extras_pass"]["median_ms"]
    ex_all = t["all_extras"]["median_ms"] - t["no_extras_pass"]["median_ms"]
    ex_all_min = t["all_extras"]["min_ms"] - t["no_extras_pass"]["min_ms"]   # (medians of the all-live call can be pool growth)
    res["extras"] = dict(t, extras_pass_all_live_from_minima_ms=ex_all_min,
                         live_share_from_minima_ms=listed / npx * ex_all_min,
                         extras_pass_over_live_share_from_minima=ex / (listed / npx * ex_all_min) if listed else None,
                         capacity_rays=npx * (mx - pre), live_rays=listed * (mx - pre),
                         live_fraction=listed / npx, extras_pass_ms=ex, extras_pass_all_live_ms=ex_all,
                         live_share_of_all_live_ms=listed / npx * ex_all,
                         extras_pass_over_live_share=ex / (listed / npx * ex_all) if listed else None)
    print("extras", json.dumps(res["extras"]), flush=True)
    for q in (r, r_none, r_all):
        q.sync(s.cuda_stream)
        q.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
