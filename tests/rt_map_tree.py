"""Test infrastructure for tests/test_rt_map_tree.py and tests/test_gpu_rt_map.py:
ray trees expanded level by level through an ``rt_map`` callback, then summed in
RayTracer#trace_sync's order (ray_tracer.rb:16-46).

A level is a dict of arrays over its m items: ``rays`` [m, 6] = (front,
position), ``att`` [m, 3], ``keys`` int32 [m, 4] = (x, y, sample, remaining
trace_depth), ``paths`` uint64 [m].  The callback answers one rt_map call per
item with a dict of arrays shaped as rtx_rt_map's outputs: ``n_children``,
``n_leaves`` [m], ``children`` [m, CMAX, 9] = (front, position, attenuation),
``child_paths`` [m, CMAX], ``leaves`` [m, LMAX, 3] (and whatever else it likes:
the dict is kept with the level).  Every returned child is submitted to the
next level, dead ones too: rt_map is what discards them (:52).
"""

import numpy as np


def level0(rays, keys3, depth):
    """The roots trace_sync starts from (:21): attenuation ones, path 1, the full depth."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    keys3 = np.asarray(keys3, np.int32).reshape(-1, 3)
    keys = np.concatenate([keys3, np.full((len(rays), 1), depth, np.int32)], axis=1)
    return {"rays": rays, "att": np.ones((len(rays), 3)), "keys": np.ascontiguousarray(keys),
            "paths": np.ones(len(rays), np.uint64)}


def live_mask(level):
    """Items that pass rt_map's cutoff (:52): depth > 0 and not att.r < 0.0001 (Vec3#r's own sum)."""
    import math
    return np.array([d > 0 and not math.sqrt(a * a + b * b + c * c) < 0.0001
                     for (a, b, c), d in zip(level["att"].tolist(), level["keys"][:, 3].tolist())], bool)


def next_level(level, out):
    """The children ``out`` returned for ``level``, in item order then child order, as the next level's items."""
    nch = np.asarray(out["n_children"], np.int64)
    item = np.repeat(np.arange(len(nch)), nch)
    slot = np.arange(len(item)) - np.repeat(np.cumsum(nch) - nch, nch)
    ch = out["children"][item, slot]
    keys = level["keys"][item].copy()
    keys[:, 3] -= 1                                   # every child's depth is the item's - 1
    return {"rays": np.ascontiguousarray(ch[:, :6]), "att": np.ascontiguousarray(ch[:, 6:9]),
            "keys": np.ascontiguousarray(keys), "paths": np.ascontiguousarray(out["child_paths"][item, slot])}


def expand(roots, rt_map, max_levels=100):
    """Breadth-first: one callback batch per level until a level returns no child.
    -> [(level, out)] per level."""
    levels = []
    level = roots
    while len(level["rays"]):
        assert len(levels) < max_levels, "the trees do not end"
        out = rt_map(level)
        levels.append((level, out))
        level = next_level(level, out)
    return levels


def tree_sums(levels):
    """Per root: the sum of its tree's leaves in trace_sync's order -- LIFO (Array#pop, :24): a node's
    leaves, then its children visited last-pushed first -- added as rt_reduce adds them (:292-298),
    and whether any partial sum was not <= 1 in every component (rt_reduce's raise)."""
    first = [np.cumsum(out["n_children"], dtype=np.int64) - out["n_children"] for _, out in levels]
    nroot = len(levels[0][0]["rays"]) if levels else 0
    sums = np.zeros((nroot, 3))
    gt1 = np.zeros(nroot, bool)
    for r in range(nroot):
        s = [0.0, 0.0, 0.0]
        stack = [(0, r)]
        while stack:
            l, i = stack.pop()
            out = levels[l][1]
            for k in range(int(out["n_leaves"][i])):
                c = out["leaves"][i, k]
                s = [s[0] + float(c[0]), s[1] + float(c[1]), s[2] + float(c[2])]
                if not (s[0] <= 1 and s[1] <= 1 and s[2] <= 1):
                    gt1[r] = True
            f = int(first[l][i])
            stack.extend((l + 1, f + j) for j in range(int(out["n_children"][i])))
        sums[r] = s
    return sums, gt1


def max_pending(levels):
    """-> (peak [roots], live [levels]).  peak: per root, the most siblings stacked at once by a walk of
    its tree in trace_sync's order that keeps the engines' discipline (rtx_device.h emit): only the
    children that pass rt_map's cutoff (live_mask) exist for it, and of a node's live children the last
    one, the one Array#pop returns next, is held, not stacked.  A camera of trace_depth D and pt
    path-tracing children can reach (D - 1) * (1 + pt), one less than the `need` the lanes engine sizes
    its stack by.  live: the live items per level, the rays rtx_level_stats counts."""
    first = [np.cumsum(out["n_children"], dtype=np.int64) - out["n_children"] for _, out in levels]
    live = [live_mask(level) for level, _ in levels]
    nroot = len(levels[0][0]["rays"]) if levels else 0
    peak = np.zeros(nroot, np.int64)
    for r in range(nroot):
        stack, held = [], (0, r) if live[0][r] else None
        while held is not None or stack:
            l, i = held if held is not None else stack.pop()
            held = None
            f, n = int(first[l][i]), int(levels[l][1]["n_children"][i])
            kids = [(l + 1, f + j) for j in range(n) if live[l + 1][f + j]] if n else []
            if kids:
                stack.extend(kids[:-1])
                held = kids[-1]
            peak[r] = max(peak[r], len(stack))
    return peak, np.array([int(m.sum()) for m in live], np.int64)


# ------------------------------------------------------------------ the oracle as the callback
def oracle_item(level, i):
    """Item i of a level as rt_ref.RayTracer.rt_map takes it, and its (x, y, sample)."""
    from oracle import rt_ref
    from oracle.rb_vec3 import Vec3
    v = [float(t) for t in level["rays"][i]]          # Python floats: Plane#intersect fails on numpy booleans
    a = [float(t) for t in level["att"][i]]
    x, y, sample, depth = (int(t) for t in level["keys"][i])
    return (rt_ref.Ray(Vec3(*v[:3]), Vec3(*v[3:])), depth, Vec3(*a), int(level["paths"][i])), x, y, sample


def oracle_rt_map(tracer, on_item=None):
    """The callback running rt_ref.RayTracer.rt_map (``tracer``) item by item.  A raise is recorded
    as ``raised`` [m] (the RtxError's kind, else None) with no children and no leaves.
    on_item(level, i, call) wraps each call (e.g. to count libm calls) and returns its result."""
    from oracle.rb_vec3 import RtxError
    cmax, lmax = 2 + tracer.pt_times, max(len(tracer.world.lights), 1)

    def cb(level):
        m = len(level["rays"])
        out = {"n_children": np.zeros(m, np.int32), "n_leaves": np.zeros(m, np.int32),
               "children": np.zeros((m, cmax, 9)), "child_paths": np.zeros((m, cmax), np.uint64),
               "leaves": np.zeros((m, lmax, 3)), "raised": [None] * m}
        for i in range(m):
            item, x, y, sample = oracle_item(level, i)
            call = lambda: tracer.rt_map(item, x, y, sample)
            try:
                children, leaves = on_item(level, i, call) if on_item else call()
            except RtxError as e:
                out["raised"][i] = e.kind
                continue
            out["n_children"][i], out["n_leaves"][i] = len(children), len(leaves)
            for k, (ray, depth, att, path) in enumerate(children):
                assert depth == item[1] - 1
                out["children"][i, k] = ray.front.to_a() + ray.position.to_a() + att.to_a()
                out["child_paths"][i, k] = path
            for k, c in enumerate(leaves):
                out["leaves"][i, k] = c.to_a()
        return out
    return cb
